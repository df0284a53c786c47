"""GPU: the fp16 weight-gradient family of csrc/wgrad_f16x3.hip -- the per-tap wgrad_f16x3_kernel, the filter-row
wgrad_f16x3_row_kernel<1|3|5> (LDS-DMA ring three chunks ahead, counted waits, XCD remap) and the strided entry -- under EVERY
form, split and edge, forced through the library's selectors (F.tuning: wg3_row, wg3_split) and called through the C ABI.
Shapes, the planners' arithmetic and the inputs: tests/wg3_cases.py (pinned on the CPU by tests/test_wg3_plan_abi.py, which also
checks that the case table reaches row splits of exactly 1, 2 and 3 chunks -- where the ring's prologue already re-fetches the
last chunk --, splits that start mid image row and on an image boundary, idle workgroups with several workgroups per XCD, and
per-tap launches of one chunk, two chunks, an odd and an even loop).

Three kinds of inputs per case:
  * "int": integers in [-8, 8] with one element of each operand pinned to +-8.  The first fp16 plane is exact, the second zero,
    every partial sum is an integer below 2^24 times a power of two: the result is EXACT whatever the summation order.  Every
    slab [split][tap] must equal conv_ref.conv2d_dw restricted to that split's pixels [16 q_begin, 16 q_end), every bias_part row
    the column sums of dy over them -- value for value (a chunk summed into the wrong split, a chunk dropped or counted twice, a
    halo shifted by a pixel cannot hide in a tolerance or in the total).
  * "resid": x = (m + 0.45) 2^-3, dy = (n + 0.45) 2^5 with m, n integers in [1024, 1100]: all positive, every element's second
    plane is +0.45 units of the first one's last place, so each cross product a1.b0 / a0.b1 carries about 4e-4 of EVERY output
    with one sign (emulated on the CPU: dropping either moves every output by >= 3e-4).  Against float64 of the fp32 inputs.
  * "rnd": the uniform zero-mean inputs of tests/test_hip_f16x3.py; on one shape per form also "spread": dy's channel k scaled by
    2^(-20 k / (K - 1)) under ONE scale record (the operand magnitudes of test_hip_dynrange.test_weight_gradients_per_channel).
Gate of the last three: the sum of the slabs within 1e-4 of the maximum of the output's OWN (tap, k) row, no floor (north_star's
bound, per row instead of per tensor); rows whose reference is all zero (filter rows that never meet the image) must be exact
zeros; the unpacked dw (stem_unpack_wgrad) takes the same bound per k; the bias gradient within 1e-4 of the sum of its terms'
magnitudes (test_hip_fp32_plans.per_sum).

Around every launch: slabs and bias_part are NaN-filled and sit inside larger buffers, 256 sentinel floats before and after must
stay bit-unchanged and no NaN may survive inside (every element of [splits][T][K][C] and [splits][K] is written, nothing past
them is); a second launch into fresh buffers is bit-identical; a third one with bias_part = NULL leaves the slabs bit-identical
and a poisoned bias buffer untouched; stem_tuning_get("wg3_ran_form" | "wg3_ran_taps" | "wg3_ran_split") equals the restatement.

Measured on the MI355X: every integer case is exact in every form; worst err / own row maximum per-tap 1.8e-6, row S = 1 / 3 / 5
6.1e-7 / 1.8e-6 / 5.8e-7, strided 1.5e-6; the whole file takes 5 s.
"""
import functools

import numpy as np
import pytest
import torch

import conv_ref as ref
import wg3_cases as W3
from test_hip_fp32_plans import SENT, dev, rnd, spread

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

GUARD = 256
NAN_BITS = 0x7FC00000
WORST = {}                 # form -> worst err / own (tap, k) row maximum seen (printed when the module is done)
INT_EXACT = {}             # form -> every integer case so far was exact


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield functional
    for form in sorted(WORST):
        print(f"[wg3 forms] worst err / own (tap, k) row maximum, {form}: {WORST[form]:.2e}; integer cases exact: {INT_EXACT.get(form)}")


@pytest.fixture(scope="module")
def lib(F):
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def s1(B, C, H, W, K, R, S=None, pad=None):
    S = R if S is None else S
    return ("s1", B, C, H, W, K, R, S, 1, R // 2 if pad is None else pad)


def strided(B, C, H, W, K, R, st, pad):
    return ("strided", B, C, H, W, K, R, R, st, pad)


ROW = {n: s1(*g) for n, g in W3.ROW_SHAPES.items()}
TAP = {n: s1(*g) for n, g in W3.TAP_SHAPES.items()}
STR = {n: strided(*g) for n, g in W3.STRIDED_SHAPES.items()}
SPREAD_ON = (ROW["3x3_ring_wraps"], TAP["33_chunks_ragged"], STR["s2_odd_fine_grid"])


def plan(g, sel, forced):
    """(wg3_ran_form, wg3_ran_taps, wg3_ran_split) the restatement expects"""
    entry, B, C, H, W, K, R, S, st, pad = g
    if entry == "strided":
        return 1, 0, W3.splits_strided(B, C, H, W, K, R, S, st, pad, forced)
    rows = W3.row_form(H, W, R, S, pad, sel)
    return (2 if rows else 1), (S if rows else 0), W3.splits_s1(B, C, H, W, K, R, S, pad, sel, forced)


def form_name(g, form, taps):
    return "strided" if g[0] == "strided" else f"row S={taps}" if form == 2 else "per-tap"


# ---- inputs and references (computed once per geometry, shared, never modified) ---------------------------------------------------
XWIDE, DYWIDE = (32, 64), (64, 96)        # channel views: (first channel, channels added) of the wider planes tensors


@functools.lru_cache(maxsize=None)
def operands(g, kind, views=False, swapped=False):
    """(x [B, C + .., H, W] on the fine grid, dy [B, K + .., OH, OW] on the coarse one) as fp32 arrays; `swapped`: other draws for
    the transposed layer's role"""
    entry, B, C, H, W, K, R, S, st, pad = g
    OH, OW = W3.out_hw(H, W, R, S, st, pad)
    Cw, Kw = C + (XWIDE[1] if views else 0), K + (DYWIDE[1] if views else 0)
    xs, ds, sd = (B, Cw, H, W), (B, Kw, OH, OW), 100 if swapped else 0
    if kind == "int":
        x, dy = W3.ints(xs, 71 + sd, 8.0), W3.ints(ds, 72 + sd, -8.0)
    elif kind == "resid":
        x, dy = W3.resid(xs, 73 + sd, W3.X_EXP), W3.resid(ds, 74 + sd, W3.DY_EXP)
    elif kind == "rnd":
        x, dy = rnd(xs, 51 + sd, -2, 2), rnd(ds, 52 + sd)
    else:
        x, dy = rnd(xs, 41 + sd), (rnd(ds, 42 + sd) * spread(Kw)[None, :, None, None]).astype(np.float32)
    for a in (x, dy):
        a.setflags(write=False)
    return x, dy


def narrow(g, x, dy, views):
    C, K = g[2], g[5]
    return (x[:, XWIDE[0]:XWIDE[0] + C], dy[:, DYWIDE[0]:DYWIDE[0] + K]) if views else (x, dy)


def dw_of(g, x, dy, swapped):
    """[K, C, R, S] in float64: the Conv2d's weight gradient, or the ConvTranspose2d's (its input on the coarse grid plays dy, the
    gradient of its output on the fine grid plays x; weight [Cin = K][Cout = C])"""
    R, S, st, pad = g[6:]
    return ref.deconv2d_dw(dy, x, R, S, st, pad) if swapped else ref.conv2d_dw(x, dy, R, S, st, pad)


@functools.lru_cache(maxsize=None)
def reference(g, kind, views=False, swapped=False):
    x, dy = narrow(g, *operands(g, kind, views, swapped), views)
    dw = dw_of(g, x, dy, swapped)
    T, K, C = g[6] * g[7], g[5], g[2]
    return dict(dw=dw, slab=np.ascontiguousarray(dw.transpose(2, 3, 0, 1).reshape(T, K, C)), db=ref.bias_grad(dy),
                l1=np.abs(dy.astype(np.float64)).sum(axis=(0, 2, 3)))


@functools.lru_cache(maxsize=None)
def split_reference(g, splits, views=False, swapped=False):
    """integer inputs: ([splits][T][K][C], [splits][K]) -- the weight gradient and dy's column sums restricted to each split's pixels"""
    entry, B, C, H, W, K, R, S, st, pad = g
    x, dy = narrow(g, *operands(g, "int", views, swapped), views)
    OH, OW = dy.shape[2:]
    M = B * OH * OW
    slabs, bias = np.zeros((splits, R * S, K, C)), np.zeros((splits, K))
    for z, (qb, qe) in enumerate(W3.chunk_ranges(W3.nchunks_of(B, OH, OW), splits)):
        m0, m1 = qb * W3.PX, min(qe * W3.PX, M)
        live = np.zeros(M, bool)
        live[m0:m1] = True
        b0, b1 = m0 // (OH * OW), (m1 - 1) // (OH * OW) + 1              # the images the split touches
        dyz = (dy * live.reshape(B, 1, OH, OW))[b0:b1]
        slabs[z] = dw_of(g, x[b0:b1], dyz, swapped).transpose(2, 3, 0, 1).reshape(R * S, K, C)
        bias[z] = ref.bias_grad(dyz)
    return slabs, bias


# ---- launches -------------------------------------------------------------------------------------------------------------------
class Guarded:
    """n floats of NaN between two runs of GUARD sentinel floats"""
    def __init__(self, n):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENT, device="cuda", dtype=torch.float32)
        self.body = self.buf[GUARD:GUARD + n]
        self.body.fill_(float("nan"))
        assert int(self.body.view(torch.int32)[0].item()) == NAN_BITS

    @property
    def ptr(self):
        return self.body.data_ptr()

    def guards_intact(self):
        b = self.buf.view(torch.int32)
        sent = int(np.float32(SENT).view(np.int32))
        return bool((b[:GUARD] == sent).all().item()) and bool((b[GUARD + self.n:] == sent).all().item())

    def untouched(self):
        return self.guards_intact() and bool((self.body.view(torch.int32) == NAN_BITS).all().item())

    def bits(self):
        return self.body.view(torch.int32)


def call(F, lib, g, xp, dyp, dw_ptr, bias_ptr, splits, **over):
    entry, B, C, H, W, K, R, S, st, pad = g
    a = dict(xpix=xp.pix_bytes, dypix=dyp.pix_bytes, B=B, H=H, W=W, C=C, K=K, R=R, S=S, st=st, pad=pad)
    a.update(over)
    head = (xp.data_ptr(), xp.q_ptr(), a["xpix"], dyp.data_ptr(), dyp.q_ptr(), a["dypix"], dw_ptr, bias_ptr, a["B"], a["H"], a["W"], a["C"], a["K"],
            a["R"], a["S"])
    if entry == "strided":
        return lib.stem_conv2d_wgrad_f16x3_strided(*head, a["st"], a["pad"], splits, F._stream())
    return lib.stem_conv2d_wgrad_f16x3(*head, a["pad"], splits, F._stream())


def query(lib, g):
    entry, B, C, H, W, K, R, S, st, pad = g
    if entry == "strided":
        return int(lib.stem_wgrad_f16x3_strided_splits(B, H, W, C, K, R, S, st, pad))
    return int(lib.stem_wgrad_f16x3_splits(B, H, W, C, K, R, S, pad))


def ran(lib):
    return tuple(int(lib.stem_tuning_get(k)) for k in (b"wg3_ran_form", b"wg3_ran_taps", b"wg3_ran_split"))


def per_row(got, want, what, form):
    """every (tap, k) row within 1e-4 of ITS OWN maximum, no floor; rows whose reference is all zero must be exact zeros"""
    cmax, err = np.abs(want).max(axis=-1), np.abs(got - want).max(axis=-1)
    dead = cmax == 0
    assert not np.abs(got[dead]).any(), f"{what}: a row whose taps never meet the image is not all zero"
    assert not dead.all(), what
    ratio = err[~dead] / cmax[~dead]
    print(f"[per row] {what}: worst err / own row max {ratio.max():.2e}, tensor max {cmax.max():.2e}")
    WORST[form] = max(WORST.get(form, 0.0), float(ratio.max()))
    assert (ratio <= 1e-4).all(), f"{what}: worst row {ratio.max():.3e} of its own maximum; {int((ratio > 1e-4).sum())} of {ratio.size} rows beyond 1e-4"


def describe(bad):
    idx = np.argwhere(bad)
    return (f"{len(idx)} of {bad.size} slab elements differ from the exact integer result, first at [split, tap, k, c] = {idx[0].tolist()}; "
            f"(split, tap) slabs with a difference: {sorted({(int(a), int(b)) for a, b in idx[:, :2]})[:12]}")


def run_case(F, lib, g, sel=0, forced=0, kinds=("int", "resid", "rnd"), views=False, bias=True, swapped=False, keep=None):
    """one forced plan, every kind of input; `keep`: a dict that receives the first launch's slab bits per kind"""
    entry, B, C, H, W, K, R, S, st, pad = g
    T = R * S
    want_form, want_taps, splits = plan(g, sel, forced)
    form = form_name(g, want_form, want_taps)
    kinds = tuple(kinds) + (("spread",) if g in SPREAD_ON and not views and "rnd" in kinds else ())
    with F.tuning(wg3_row=sel, wg3_split=forced):
        assert query(lib, g) == splits, (g, sel, forced, query(lib, g), splits)
        for kind in kinds:
            what = f"{g} wg3_row {sel} wg3_split {forced} ({splits} splits) {kind}{' views' if views else ''}{' transposed role' if swapped else ''}"
            x, dy = operands(g, kind, views, swapped)
            xp, dyp = F.F16Planes.split(dev(x)), F.F16Planes.split(dev(dy))
            if views:
                xp, dyp = xp.channels(XWIDE[0], XWIDE[0] + C), dyp.channels(DYWIDE[0], DYWIDE[0] + K)
                assert xp.pix_bytes > (C // 32) * 128 and dyp.pix_bytes > (K // 32) * 128 and xp.byte_offset == 128 and dyp.byte_offset == 256
            runs = []
            for with_bias in ((True, True, False) if bias else (False, False)):
                dwb, bb = Guarded(splits * T * K * C), Guarded(splits * K)
                rc = call(F, lib, g, xp, dyp, dwb.ptr, bb.ptr if with_bias else None, splits)
                assert rc == 0, (what, lib.stem_last_error())
                assert ran(lib) == (want_form, want_taps, splits), (what, ran(lib))
                runs.append((dwb, bb, with_bias))
            torch.cuda.synchronize()
            for i, (dwb, bb, with_bias) in enumerate(runs):
                assert dwb.guards_intact(), f"{what}: launch {i} wrote outside [splits][T][K][C]"
                assert not bool(torch.isnan(dwb.body).any().item()), f"{what}: launch {i} left slab elements unwritten"
                if with_bias:
                    assert bb.guards_intact(), f"{what}: launch {i} wrote outside bias_part [splits][K]"
                    assert not bool(torch.isnan(bb.body).any().item()), f"{what}: launch {i} left bias_part elements unwritten"
                else:
                    assert bb.untouched(), f"{what}: bias_part = NULL, yet the poisoned buffer changed"
                assert torch.equal(dwb.bits(), runs[0][0].bits()), f"{what}: slabs of launch {i} differ from the first launch's"
                if with_bias:
                    assert torch.equal(bb.bits(), runs[0][1].bits()), f"{what}: bias_part of launch {i} differs from the first launch's"
            slabs = runs[0][0].body.cpu().numpy().reshape(splits, T, K, C)
            bpart = runs[0][1].body.cpu().numpy().reshape(splits, K) if bias else None
            if keep is not None:
                keep[kind] = slabs.copy()
            r = reference(g, kind, views, swapped)
            if kind == "int":
                ws, wb = split_reference(g, splits, views, swapped)
                assert np.abs(ws).max() < 2 ** 24
                bad = slabs != ws.astype(np.float32)
                INT_EXACT[form] = INT_EXACT.get(form, True) and not bad.any()
                assert not bad.any(), f"{what}: {describe(bad)}"
                if bias:
                    assert np.array_equal(bpart, wb.astype(np.float32)), f"{what}: bias_part rows differ from dy's column sums over each split's pixels"
                continue
            per_row(slabs.astype(np.float64).sum(0), r["slab"], what, form)
            dw = torch.full((K, C, R, S), float("nan"), device="cuda")
            assert lib.stem_unpack_wgrad(runs[0][0].ptr, dw.data_ptr(), K, C, R, S, splits, 0, F._stream()) == 0, lib.stem_last_error()
            per_row(dw.cpu().numpy().astype(np.float64).reshape(K, -1), r["dw"].reshape(K, -1), what + " unpacked", form)
            if bias:
                ratio = np.abs(bpart.astype(np.float64).sum(0) - r["db"]) / r["l1"]
                print(f"[per sum] {what} bias: worst err / sum of |terms| {ratio.max():.2e}")
                assert (ratio <= 1e-4).all(), f"{what}: bias gradient {ratio.max():.3e} of the sum of its terms' magnitudes"


# ---- the cases ------------------------------------------------------------------------------------------------------------------
ROW_CASES = [(n, f) for n in ROW for f in W3.row_forced_list(n)]
TAP_CASES = [(n, f) for n in TAP for f in W3.tap_forced_list(n)]


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: f"{c[0]}-s{c[1]}")
def test_filter_row_form_under_every_split(F, lib, case):
    """wg3_split in {1, 2, 3, 5, n, n + 7} (n = the chunk count; the row planner clamps a forced split only to it): splits of 1, 2
    and 3 chunks, splits that start mid row / on an image boundary, filter rows outside the image, H = 1, one live wavefront,
    idle workgroups"""
    name, forced = case
    g = ROW[name]
    assert plan(g, 0, forced)[:2] == (2, g[6])
    run_case(F, lib, g, 0, forced)


@pytest.mark.parametrize("case", TAP_CASES, ids=lambda c: f"{c[0]}-s{c[1]}")
def test_per_tap_form_under_every_split(F, lib, case):
    """one partial chunk, two chunks, 17 + 16 chunks, dead wavefronts, pad != R / 2, R != S; whatever wg3_row says (0 here)"""
    name, forced = case
    g = TAP[name]
    assert plan(g, 0, forced)[:2] == (1, 0)
    run_case(F, lib, g, 0, forced)


@pytest.mark.parametrize("name", list(ROW))
def test_row_shapes_on_the_per_tap_form(F, lib, name):
    """wg3_row = 1: the same layers on the per-tap kernel (at most 16 chunks: never split, a forced split is clamped to 1)"""
    assert plan(ROW[name], 1, 3) == (1, 0, 1)
    run_case(F, lib, ROW[name], 1, 3)


@pytest.mark.parametrize("sel", [3, 6])
def test_row_selector_routing(F, lib, sel):
    """wg3_row = 3: a 3 x 3 and a 1 x 1 layer run per tap, a 5 x 5 layer as rows; wg3_row = 6: only the 1 x 1 layer leaves the row form"""
    want = {3: {"3x3_ring_wraps": 1, "1x1_three_k_tiles": 1, "5x5_idle_workgroup": 2}, 6: {"3x3_ring_wraps": 2, "1x1_three_k_tiles": 1, "5x5_idle_workgroup": 2}}[sel]
    for name, form in want.items():
        assert plan(ROW[name], sel, 2)[0] == form, (name, sel)
        run_case(F, lib, ROW[name], sel, 2, kinds=("int", "resid"))


STRIDED_CASES = [(n, 2 if n == "s2_two_splits" else 0) for n in STR]


@pytest.mark.parametrize("swapped", [False, True], ids=["conv2d", "convtranspose2d"])
@pytest.mark.parametrize("case", STRIDED_CASES, ids=lambda c: f"{c[0]}-s{c[1]}")
def test_strided_entry_in_both_roles(F, lib, case, swapped):
    """nn.Conv2d (with the bias gradient's first stage), and nn.ConvTranspose2d with the operands swapped against
    conv_ref.deconv2d_dw (no bias: bias_part = NULL); strides 1 .. 4, an odd fine grid, fine pixels no tap reads"""
    name, forced = case
    g = STR[name]
    assert not forced or plan(g, 0, forced)[2] == forced
    run_case(F, lib, g, 0, forced, bias=not swapped, swapped=swapped)


def test_strided_entry_at_stride_1_is_the_stride_1_entry(F, lib):
    """bit for bit, slab by slab, under wg3_row = 1 (both are wgrad_f16x3_kernel with the same arguments)"""
    a, b = {}, {}
    run_case(F, lib, STR["s1_is_the_stride1_entry"], 1, 2, keep=a)
    run_case(F, lib, TAP["33_chunks_ragged"], 1, 2, keep=b)
    assert STR["s1_is_the_stride1_entry"][1:] == TAP["33_chunks_ragged"][1:]
    for kind in ("int", "resid", "rnd"):
        assert a[kind].shape[0] == 2 and np.array_equal(a[kind].view(np.uint32), b[kind].view(np.uint32)), kind


@pytest.mark.parametrize("case", [("row", ROW["5x5_rows_outside"], 0, 3), ("row", ROW["3x3_ring_wraps"], 0, 5), ("tap", TAP["33_chunks_ragged"], 0, 2),
                                  ("tap", ROW["3x3_ring_wraps"], 1, 1), ("strided", STR["s2_two_splits"], 0, 2)], ids=["row5x5-s3", "row3x3-s5", "tap-s2", "tap-16chunks", "strided-s2"])
def test_channel_views(F, lib, case):
    """x as channels [32, 32 + C) of a planes tensor 64 channels wider, dy as channels [64, 64 + K) of one 96 wider: a non-zero
    first slab and a pixel pitch greater than the channels, the record of the whole tensor; both forms, with bias, at a forced
    split, and through the strided entry"""
    _, g, sel, forced = case
    run_case(F, lib, g, sel, forced, views=True)


def test_refusals_name_their_argument_and_launch_nothing(F, lib):
    g = TAP["two_chunks"]
    entry, B, C, H, W, K, R, S, st, pad = g
    x, dy = operands(g, "int")
    xp, dyp = F.F16Planes.split(dev(x)), F.F16Planes.split(dev(dy))
    gs = strided(B, C, H, W, K, R, 1, pad)
    dwb, bb = Guarded(4 * 30 * K * C), Guarded(4 * K)
    assert call(F, lib, g, xp, dyp, dwb.ptr, bb.ptr, 1) == 0
    torch.cuda.synchronize()
    before = ran(lib)
    dwb, bb = Guarded(4 * 30 * K * C), Guarded(4 * K)
    for what, gg, splits, over, words in (
            ("splits not the planner's", g, 2, {}, (b"splits", b"stem_wgrad_f16x3_splits")),
            ("splits not the planner's (strided)", gs, 2, {}, (b"splits", b"stem_wgrad_f16x3_strided_splits")),
            ("C = 48", g, 1, dict(C=48), (b"C % 32 == 0", b"C=48")),
            ("R * S = 30", g, 1, dict(R=5, S=6, pad=2), (b"R*S <= 25", b"R=5 S=6")),
            ("stride 5", gs, 1, dict(st=5), (b"1 <= stride <= 4", b"stride=5")),
            ("stride 0", gs, 1, dict(st=0), (b"1 <= stride <= 4", b"stride=0")),
            ("x pitch not a multiple of 128", g, 1, dict(xpix=(C // 32) * 128 + 64), (b"pixel pitches", b"128")),
            ("dy pitch below the channels", gs, 1, dict(dypix=(K // 32 - 1) * 128), (b"pixel pitches", b"128"))):
        with F.tuning(wg3_row=0, wg3_split=0):
            rc = call(F, lib, gg, xp, dyp, dwb.ptr, bb.ptr, splits, **over)
        err = lib.stem_last_error()
        assert rc != 0 and all(w in err for w in words), (what, rc, err)
        assert ran(lib) == before, what
    torch.cuda.synchronize()
    assert dwb.untouched() and bb.untouched(), "a refused call wrote to its outputs"
