"""GPU: the block kernels of csrc/resblock.hip against tests/cheng_ref.py -- the pixel shuffle (with its folded leaky ReLU and
addend) and add_act bit for bit, forward and backward; the gate inside the bound derived in cheng_ref from its roundings and the
device expf's documented error, against float64."""
import numpy as np
import pytest
import torch

import cheng_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.detach().cpu().numpy()


def _values(seed, shape):
    """normal values with exact zeros, negative zeros and tiny numbers mixed in"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape).astype(np.float32)
    flat = v.reshape(-1)
    n = flat.size
    flat[rng.integers(0, n, max(1, n // 7))] = 0.0
    flat[rng.integers(0, n, max(1, n // 11))] = -0.0
    flat[rng.integers(0, n, max(1, n // 13))] = np.float32(1e-40)
    return v


def _nhwc(a, pad=0, off=0):
    """numpy [B, H, W, C] -> logical [B, C, H, W] tensor on the device with NHWC memory; pad > 0: a channel-slice view starting at
    channel `off` of a buffer with pitch C + pad whose other channels hold NaN"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if not pad:
        return t.permute(0, 3, 1, 2)
    B, H, W, C = a.shape
    buf = torch.full((B, H, W, C + pad), float("nan"), device=DEV, dtype=torch.float32)
    view = buf.permute(0, 3, 1, 2)[:, off:off + C]
    view.copy_(t.permute(0, 3, 1, 2))
    return view


def _back(t):
    """logical [B, C, H, W] (any strides) -> numpy [B, H, W, C]"""
    return host(t.permute(0, 2, 3, 1).contiguous())


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _shuffle_case(r, C, shape, addend, slope, sliced, seed):
    from spatiotemporalentropymodel_amd import functional as F
    B, H, W = shape
    x = _values(seed, (B, H, W, C * r * r))
    add = _values(seed + 1, (B, H * r, W * r, C)) if addend else None
    g = _values(seed + 2, (B, H * r, W * r, C))
    # 16-byte path (C % 4 == 0): pitches stay multiples of 4 and slices start on a 16-byte boundary; otherwise anything goes
    pad, off = ((8, 4) if C % 4 == 0 else (5, 1)) if sliced else (0, 0)
    xt, at, gt = _nhwc(x, pad, off), (_nhwc(add, pad, off) if addend else None), _nhwc(g, pad, off)
    what = f"r={r} C={C} shape={shape} addend={addend} slope={slope} sliced={sliced}"
    out = None
    if sliced:                                                   # the output as a channel slice too: the neighbours stay untouched
        buf = torch.full((B, H * r, W * r, C + pad), 7.0, device=DEV)
        out = buf.permute(0, 3, 1, 2)[:, off:off + C]
    y = F.pixel_shuffle(xt, r, slope, at, out=out)
    assert tuple(y.shape) == (B, C, H * r, W * r), what
    assert _same_bits(_back(y), R.pixel_shuffle_fwd(x, r, slope, add)), "forward: " + what
    if sliced:
        rest = host(buf)
        assert np.all(rest[..., :off] == 7.0) and np.all(rest[..., off + C:] == 7.0), "forward wrote outside its slice: " + what
    din = F.pixel_shuffle_backward(gt, r, xt, slope)
    assert tuple(din.shape) == (B, C * r * r, H, W), what
    assert _same_bits(_back(din), R.pixel_shuffle_bwd(g, r, x, slope)), "backward: " + what
    if slope == 1.0:
        assert _same_bits(_back(F.pixel_shuffle_backward(gt, r)), R.pixel_shuffle_bwd(g, r)), "backward without x: " + what


SHAPES = [(1, 1, 1), (2, 3, 5), (1, 7, 33)]


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("C", [3, 4, 8, 36, 192])
def test_pixel_shuffle_bit_for_bit(r, C):
    """(1, 7, 33) with C = 192: 4 (r = 2) or 2 (r = 3) pixels per LDS segment, a partial one at the end of every row"""
    seed = 1000 * r + C
    for shape in SHAPES:
        for addend in (False, True):
            for slope in (1.0, 0.01):
                for sliced in (False, True):
                    _shuffle_case(r, C, shape, addend, slope, sliced, seed)
                    seed += 3
    torch.cuda.synchronize()


@pytest.mark.parametrize("r,C,shape,why", [
    (2, 8, (1, 2, 70), "segments capped at 64 pixels: a second, partial segment of 6"),
    (1, 4, (1, 1, 200), "r = 1: a plain copy, four segments"),
    (9, 192, (1, 2, 3), "one pixel's 15552 floats exceed the LDS budget: two channel chunks (148 + 44 channels), one pixel per segment"),
    (60, 4, (1, 1, 2), "a 4-channel chunk no longer fits: the direct kernel although C % 4 == 0"),
    (2, 1, (2, 5, 9), "C = 1"),
    (2, 3, (1, 16, 24), "the last layer of g_s: 12 -> 3 channels")])
def test_pixel_shuffle_other_paths(r, C, shape, why):
    for k, (addend, slope, sliced) in enumerate(((True, 0.01, False), (False, 1.0, True), (True, 0.2, True))):
        _shuffle_case(r, C, shape, addend, slope, sliced, 77 + 10 * k)
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [3, 8, 192])
@pytest.mark.parametrize("slope", [0.0, 0.01])
def test_add_act_bit_for_bit(C, slope):
    from spatiotemporalentropymodel_amd import functional as F
    for shape in ((1, 1, 1), (2, 3, 5), (1, 9, 31)):
        for sliced in (False, True):
            a, g = _values(C + 1, (*shape, C)), _values(C + 3, (*shape, C))
            b = _values(C + 2, (*shape, C))
            b.reshape(-1)[::5] = -a.reshape(-1)[::5]                           # sums that are exactly zero
            pad, off = ((8, 4) if C % 4 == 0 else (5, 1)) if sliced else (0, 0)
            at, bt, gt = _nhwc(a, pad, off), _nhwc(b, pad, off), _nhwc(g, pad, off)
            out = F.add_act(at, bt, slope)
            ref = R.add_act_fwd(a, b, slope)
            assert (ref == 0).sum() >= ref.size // 5 and (ref.size < 50 or (ref < 0).any() == (slope > 0))
            assert _same_bits(_back(out), ref), (C, slope, shape, sliced)
            grad = F.add_act_backward(out, gt, slope)
            assert _same_bits(_back(grad), R.add_act_bwd(ref, g, slope)), (C, slope, shape, sliced)
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [3, 24])
def test_gate_within_the_derived_bound(C):
    from spatiotemporalentropymodel_amd import functional as F
    rng = np.random.default_rng(C)
    shape = (2, 6, 10, C)
    a, x, g = (rng.uniform(-2, 2, shape).astype(np.float32) for _ in range(3))
    b = rng.uniform(-30, 30, shape).astype(np.float32)
    b.reshape(-1)[:12] = [30.0, -30.0, 0.0, -0.0, 1e-3, -1e-3, 17.5, -17.5, 88.0, -88.0, 200.0, -200.0]
    for sliced in (False, True):
        pad, off = ((8, 4) if C % 4 == 0 else (5, 1)) if sliced else (0, 0)
        at, bt, xt, gt = (_nhwc(v, pad, off) for v in (a, b, x, g))
        out = _back(F.gate(at, bt, xt)).astype(np.float64)
        err = np.abs(out - R.gate_fwd(a, b, x, np.float64))
        bound = R.gate_fwd_bound(a, b, x)
        print(f"[gate C={C} sliced={sliced}] forward: worst error / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound), float((err / bound).max())
        da, db = F.gate_backward(at, bt, gt)
        da64, db64 = R.gate_bwd(a, b, g, np.float64)
        bda, bdb = R.gate_bwd_bounds(a, b, g)
        eda, edb = np.abs(_back(da) - da64), np.abs(_back(db) - db64)
        print(f"[gate C={C} sliced={sliced}] backward: worst error / bound da {float((eda / bda).max()):.3f}, db {float((edb / bdb).max()):.3f}")
        assert np.all(np.isfinite(_back(db))) and np.all(eda <= bda) and np.all(edb <= bdb)
    torch.cuda.synchronize()


def test_autograd_functions():
    """PixelShuffleFunction / AddActFunction / GateFunction: the gradients autograd hands out are the backward kernels' (and dout
    itself for the addend and the gate's x), for NCHW-contiguous inputs too"""
    from spatiotemporalentropymodel_amd import layers as L
    r, C, B, H, W = 2, 8, 2, 3, 5
    x, add, g = _values(1, (B, H, W, C * r * r)), _values(2, (B, H * r, W * r, C)), _values(3, (B, H * r, W * r, C))
    xt = _nhwc(x).contiguous().requires_grad_(True)                              # NCHW memory: converted inside the Function
    at = _nhwc(add).detach().requires_grad_(True)
    y = L.PixelShuffleFunction.apply(xt, r, 0.01, at)
    assert _same_bits(_back(y), R.pixel_shuffle_fwd(x, r, 0.01, add))
    y.backward(_nhwc(g))
    assert _same_bits(_back(xt.grad), R.pixel_shuffle_bwd(g, r, x, 0.01)) and _same_bits(_back(at.grad), g)
    a, b = _values(4, (B, H, W, C)), _values(5, (B, H, W, C))
    ta, tb = _nhwc(a).detach().requires_grad_(True), _nhwc(b).contiguous().requires_grad_(True)
    out = L.AddActFunction.apply(ta, tb, 0.0)
    d = _values(6, (B, H, W, C))
    out.backward(_nhwc(d))
    ref = R.add_act_bwd(R.add_act_fwd(a, b, 0.0), d, 0.0)
    assert _same_bits(_back(ta.grad), ref) and _same_bits(_back(tb.grad), ref)
    ta, tb, tx = (_nhwc(v).detach().requires_grad_(True) for v in (a, b * 10, d))
    L.GateFunction.apply(ta, tb, tx).backward(_nhwc(add[:, :H, :W]))
    da64, db64 = R.gate_bwd(a, b * 10, add[:, :H, :W], np.float64)
    bda, bdb = R.gate_bwd_bounds(a, b * 10, add[:, :H, :W])
    assert np.all(np.abs(_back(ta.grad) - da64) <= bda) and np.all(np.abs(_back(tb.grad) - db64) <= bdb)
    assert _same_bits(_back(tx.grad), add[:, :H, :W])
    torch.cuda.synchronize()
