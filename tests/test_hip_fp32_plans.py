"""GPU: the fp32-MFMA convolution family (csrc/igemm.hip) and weight-gradient family (csrc/wgrad.hip) under EVERY tile
configuration and split plan, forced through the library's selectors (F.tuning: igemm_cfg, igemm_fuse_cfg, igemm_split,
wgrad_cfg; the `splits` argument of the weight gradients) instead of left to the planners' cost models.

Every case: force a plan; size a zeroed workspace of its own with stem_conv_workspace_bytes queried under that plan (checked
against 65536 + s_eff * B*OH*OW*N*4, or 0 for s_eff = 1; s_eff = cdiv(chunks, cdiv(chunks, min(s, chunks))), chunks = taps x
cdiv(C, 32) of the phase with the most taps); call the C ABI; assert that stem_tuning_get("igemm_ran_cfg" | "igemm_ran_split" |
"wgrad_ran_cfg") reports the forced plan as the one that ran; compare with the float64 statements of tests/conv_ref.py (pinned
on the CPU by tests/test_conv_ref.py).

Gate: every channel of a result within 1e-4 of ITS OWN maximum against float64, no floor (test_hip_dynrange.per_channel, span
20).  The channel is the kernel's output channel: the layer's output channel for a forward, its input channel for an input
gradient, the output-channel row for dW.  Output channel k of the weights and of the bias carries the scale 2^(-20 k / (K - 1)),
the bias is U(-1, 1) times that scale (a lost or doubled bias is ~1e-1 of a channel), xact holds exact 0.0 and -0.0.  Vectors
that are themselves pixel sums (db, dbeta) have no channel to take a maximum over; element k is held to 1e-4 of the sum of the
magnitudes of ITS summed terms -- fp32 summation error is relative to that sum ((n - 1) eps with n <= 200 pixels here is 1.2e-5,
the terms themselves are exact (db) or a few ulp of elementwise fp32 work (dbeta)).

Exact relations asserted on top:
  * the same forced launch twice into the same workspace is bit-identical (the reduce adds the slabs in split order);
  * after every split launch the first 64 KiB of the workspace (arrival counters) are zero;
  * an output written into a channel slice of a wider NHWC buffer leaves every other channel at its sentinel;
  * bit equality ACROSS the six tile configurations at equal s_eff.  Reading igemm_kernel: an output element's accumulator is
    one chain of v_mfma_f32_32x32x2_f32 in every instantiation; the chain walks the chunks q_begin .. q_end in order (the split
    bounds come from the chunk count and the split count alone, not from the tile), inside a chunk the four k-groups and the
    four steps in the same order (k = 8 k8 + s from lanes 0-31, 8 k8 + 4 + s from lanes 32-63), zero padding (tile tails, K
    tails) adds +-0 products that do not change an accumulator that started at +0, and the bias / reduce / activation epilogues
    are per element.  The tile only decides WHICH lane holds the element.  So all six must agree to the bit, for the GDN-operand
    kernels too; the fused-GDN kernels exist in two tiles only and are compared the same way.

Exclusions -- cases the library refuses with an error (asserted below), nothing else is left out:
  * a fused conv + GDN call whose pitches rule out the vector path ("igemm: fused GDN needs 16-byte aligned ..."): the fused
    kernels exist with vector staging only.
Plans the semantics of the selectors turn into another plan by design (asserted as such, through *_ran_*):
  * the first-layer form (stem_conv2d_fwd_c4), the GDN kernels and the fused kernels never split: igemm_split is ignored;
  * fused launches take their tile from igemm_fuse_cfg and ignore igemm_cfg;
  * the folded-tap first-layer weight gradient (4-channel gathered operand) has one tile of its own, 64x64: wgrad_cfg is ignored.

Weight-gradient split counts s in {1, 2, 5} need cdiv(n, cdiv(n, s)) == s with n = cdiv(pixels, 32) chunks; the shapes below
have n = 5 (batches enlarged where the issue's layer has fewer pixels).
"""
import functools

import numpy as np
import pytest
import torch

import conv_ref as ref

pytestmark = pytest.mark.gpu

SLOPE = float(np.float32(0.01))
SENT = 3.0e9               # sentinel of output buffers: far outside every result
CNT_BYTES = 65536
ACT_LRELU, MASKED_A = 1, 0x100
WORST = {}                 # family -> worst err / own channel maximum seen (printed when the module is done)
STASH = {}                 # (case key, s_eff) -> bytes of the first configuration's result, for the cross-configuration equality


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield functional
    for fam in sorted(WORST):
        print(f"[fp32 plans] worst err / own channel maximum, {fam}: {WORST[fam]:.2e}")


@pytest.fixture(scope="module")
def lib(F):
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


def cdiv(a, b):
    return -(-a // b)


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


def spread(K, log2_span=20):
    return (2.0 ** (-log2_span * np.arange(K) / max(K - 1, 1))).astype(np.float32)


def with_zeros(a):
    """exact 0.0 and -0.0 among the values"""
    f = a.reshape(-1)
    f[::7] = 0.0
    f[3::11] = -0.0
    return a


def per_channel(a, r, what, family, axis=1, rtol=1e-4):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    assert a.shape == r.shape, (what, a.shape, r.shape)
    red = tuple(i for i in range(r.ndim) if i != axis)
    cmax, err = np.abs(r).max(axis=red), np.abs(a - r).max(axis=red)
    assert cmax.min() > 0, what
    ratio = err / cmax
    worst = int(np.argmax(ratio))
    print(f"[per channel] {what}: worst err / own max {ratio[worst]:.2e} at channel {worst} (its max {cmax[worst]:.2e}, tensor max {cmax.max():.2e})")
    WORST[family] = max(WORST.get(family, 0.0), float(ratio[worst]))
    assert (err <= rtol * cmax).all(), f"{what}: channel {worst}: err {err[worst]:.3e} > {rtol * cmax[worst]:.3e} (own max {cmax[worst]:.3e})"


def per_sum(a, r, l1, what, family, rtol=1e-4):
    """element k of a pixel sum within rtol of the sum of the magnitudes of its terms"""
    a, r, l1 = np.asarray(a, np.float64), np.asarray(r, np.float64), np.asarray(l1, np.float64)
    ratio = np.abs(a - r) / l1
    print(f"[per sum] {what}: worst err / sum of |terms| {ratio.max():.2e}")
    WORST[family] = max(WORST.get(family, 0.0), float(ratio.max()))
    assert (ratio <= rtol).all(), f"{what}: element {int(np.argmax(ratio))}: {ratio.max():.3e} of the sum of its terms' magnitudes"


# ---- NHWC buffers: a [B,C,H,W] array as a channel slice [c0, c0 + C) of a [B,H,W,ld] device buffer filled with the sentinel ----
class Buf:
    def __init__(self, shape_nchw, ld=None, c0=0, src=None):
        B, Cc, H, W = shape_nchw
        self.ld, self.c0, self.C = (Cc if ld is None else ld), c0, Cc
        assert self.c0 + Cc <= self.ld
        self.buf = torch.full((B, H, W, self.ld), SENT, device="cuda", dtype=torch.float32)
        self.view = self.buf[..., c0:c0 + Cc]
        if src is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(src, (0, 2, 3, 1)))))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def nchw(self):
        """[B,C,H,W] tensor over the same memory (what functional.py takes)"""
        return self.view.permute(0, 3, 1, 2)

    def host(self):
        return np.ascontiguousarray(np.transpose(self.view.cpu().numpy(), (0, 3, 1, 2)))

    def others_untouched(self):
        b = self.buf.cpu().numpy()
        return bool((b[..., :self.c0] == np.float32(SENT)).all() and (b[..., self.c0 + self.C:] == np.float32(SENT)).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def phase_taps(R, stride, pad):
    """taps of the sub-pixel phase with the most taps (transposed mapping, square kernels)"""
    m = max(sum(1 for r in range(R) if (p + pad - r) % stride == 0) for p in range(stride))
    return m * m


# ---- the issue's shapes ----------------------------------------------------------------------------------------------------
CONV = {
    "c40k200_3x3": dict(B=1, C=40, H=9, W=11, K=200, R=3, st=1, pad=1),           # M = 99, N tails, partial second chunk, vector
    "c37k70_5x5s2": dict(B=2, C=37, H=13, W=10, K=70, R=5, st=2, pad=2),          # scalar staging, scalar reduce with its tail
    "c64k192_1x1": dict(B=3, C=64, H=12, W=12, K=192, R=1, st=1, pad=0),          # M = 432, 2 chunks: a forced split clamps to 2
    "c32k72_maskA": dict(B=1, C=32, H=8, W=8, K=72, R=5, st=1, pad=2, mask=True),  # the 12-tap prefix
}
DECONV = {
    "c48k100": dict(B=2, C=48, H=5, W=7, K=100, R=5, st=2, pad=2, opad=1),        # four phases (9 / 6 / 6 / 4 taps), !ident mapping
    "c64k3": dict(B=2, C=64, H=5, W=7, K=3, R=5, st=2, pad=2, opad=1),            # K = 3
}
OPS = ("conv_fwd", "conv_dgrad", "deconv_fwd", "deconv_dgrad")


@functools.lru_cache(maxsize=None)
def problem(op, name):
    """operands (device, packed by the library's own pack kernels), geometry and the float64 result before the activation"""
    from spatiotemporalentropymodel_amd import functional as F
    deconv = op.startswith("deconv")
    g = dict((DECONV if deconv else CONV)[name])
    B, C, H, W, K, R, st, pad = (g[k] for k in ("B", "C", "H", "W", "K", "R", "st", "pad"))
    opad, mask = g.get("opad", 0), g.get("mask", False)
    oh, ow = ref.deconv_out_hw(H, W, R, R, st, pad, opad) if deconv else ref.conv_out_hw(H, W, R, R, st, pad)
    wshape = (C, K, R, R) if deconv else (K, C, R, R)
    p = dict(g, op=op, name=name, opad=opad, deconv=deconv, dims=(B, H, W, C, K, R, R, st, pad, opad))
    if op.endswith("fwd"):
        s = spread(K)
        w = (rnd(wshape, 2) / np.sqrt(C * R * R)).astype(np.float32) * (s[None, :, None, None] if deconv else s[:, None, None, None])
        b = rnd((K,), 3) * s
        x = rnd((B, C, H, W), 1)
        if deconv:
            pre = ref.deconv2d_fwd(x, w, b, st, pad, opad)
            taps = phase_taps(R, st, pad)
        else:
            pre = ref.conv2d_fwd(x, w * ref.mask_a(R, R) if mask else w, b, st, pad)
            taps = (R // 2) * R + R // 2 if mask else R * R
        role = F.PACK_DECONV_FWD if deconv else F.PACK_CONV_FWD
        p.update(inp=x, wp=F.pack_weight(dev(w), role, masked=1 if mask else 0), bias=dev(b), z=None, N=K, contr=C, out=(B, K, oh, ow),
                 kind=(2 if deconv else 0) | (MASKED_A if mask else 0), taps=taps, pre=pre)
    else:
        s = spread(C)                                             # the kernel's output channels are the layer's INPUT channels
        w = (rnd(wshape, 4) / np.sqrt(K * R * R)).astype(np.float32) * (s[:, None, None, None] if deconv else s[None, :, None, None])
        dy = rnd((B, K, oh, ow), 5)
        xact = with_zeros(rnd((B, C, H, W), 6))
        pre = ref.deconv2d_dx(dy, w, st, pad) if deconv else ref.conv2d_dx(dy, w, (B, C, H, W), st, pad)
        role = F.PACK_DECONV_DGRAD if deconv else F.PACK_CONV_DGRAD
        p.update(inp=dy, wp=F.pack_weight(dev(w), role), bias=None, z=xact, N=C, contr=K, out=(B, C, H, W), kind=3 if deconv else 1,
                 taps=R * R if deconv else phase_taps(R, st, pad), pre=pre)
    assert p["pre"].shape == p["out"]
    p["chunks"] = p["taps"] * cdiv(p["contr"], 32)
    return p


def s_eff_of(p, split):
    s = min(split, p["chunks"])
    return cdiv(p["chunks"], cdiv(p["chunks"], s))


def call_igemm(F, lib, p, xb, yb, zb, act, ws, wsb):
    B, H, W, C, K, R, S, st, pad, opad = p["dims"]
    wp, bias, stream = p["wp"].data_ptr(), (0 if p["bias"] is None else p["bias"].data_ptr()), F._stream()
    wsp = 0 if ws is None else ws.data_ptr()
    zp, ldz = (0, 0) if zb is None else (zb.ptr, zb.ld)
    op = p["op"]
    if op == "conv_fwd":
        return lib.stem_conv2d_fwd(xb.ptr, xb.ld, wp, bias, yb.ptr, yb.ld, B, H, W, C, K, R, S, st, pad,
                                   (ACT_LRELU if act else 0) | (MASKED_A if p.get("mask") else 0), SLOPE, wsp, wsb, stream)
    if op == "conv_dgrad":
        return lib.stem_conv2d_dgrad(xb.ptr, xb.ld, wp, yb.ptr, yb.ld, zp, ldz, SLOPE, B, H, W, C, K, R, S, st, pad, wsp, wsb, stream)
    if op == "deconv_fwd":
        return lib.stem_deconv2d_fwd(xb.ptr, xb.ld, wp, bias, yb.ptr, yb.ld, B, H, W, C, K, R, S, st, pad, opad,
                                     ACT_LRELU if act else 0, SLOPE, wsp, wsb, stream)
    return lib.stem_deconv2d_dgrad(xb.ptr, xb.ld, wp, yb.ptr, yb.ld, zp, ldz, SLOPE, B, H, W, C, K, R, S, st, pad, opad, wsp, wsb, stream)


VIEWS = {                  # name -> (input (extra pitch, offset), output (extra pitch, offset), xact (extra pitch, offset))
    None: ((0, 0), (0, 0), (0, 0)),
    "in_slice": ((8, 4), (0, 0), (0, 0)),          # ldx != C, still 16-byte rows
    "in_odd": ((5, 2), (0, 0), (0, 0)),            # ldx % 4 != 0 on a C % 4 == 0 layer: scalar staging
    "out_odd": ((0, 0), (3, 1), (5, 2)),           # ldy % 4 != 0 (and ldz): scalar reduce on an N % 4 == 0 layer
    "z_odd": ((0, 0), (0, 0), (5, 2)),             # ldz % 4 != 0 alone (the DACT reduce's own condition)
}


def run_forced(F, lib, op, name, cfg, split, act, view=None):
    p = problem(op, name)
    s_eff = s_eff_of(p, split)
    (xe, x0), (ye, y0), (ze, z0) = VIEWS[view]
    cin = p["inp"].shape[1]
    xb = Buf(p["inp"].shape, cin + xe, x0, src=p["inp"])
    zb = Buf(p["z"].shape, p["N"] + ze, z0, src=p["z"]) if (act and p["z"] is not None) else None
    what = f"{op} {name} cfg {cfg} split {split} (s_eff {s_eff}) act {act} view {view}"
    with F.tuning(igemm_cfg=cfg, igemm_split=split):
        wsb = int(lib.stem_conv_workspace_bytes(p["kind"], *p["dims"]))
        B, N, OH, OW = p["out"]
        assert wsb == (CNT_BYTES + s_eff * B * OH * OW * N * 4 if s_eff > 1 else 0), (what, wsb)
        ws = torch.zeros(wsb // 4, device="cuda", dtype=torch.int32) if wsb else None
        outs = []
        for _ in range(2 if s_eff > 1 else 1):
            yb = Buf(p["out"], N + ye, y0)
            rc = call_igemm(F, lib, p, xb, yb, zb, act, ws, wsb)
            assert rc == 0, (what, lib.stem_last_error())
            assert lib.stem_tuning_get(b"igemm_ran_cfg") == cfg, (what, lib.stem_tuning_get(b"igemm_ran_cfg"))
            assert lib.stem_tuning_get(b"igemm_ran_split") == s_eff, (what, lib.stem_tuning_get(b"igemm_ran_split"))
            outs.append(yb)
        torch.cuda.synchronize()
    got = outs[0].host()
    if s_eff > 1:
        assert int(ws[:CNT_BYTES // 4].abs().max().item()) == 0, what + ": arrival counters not left at zero"
        assert np.array_equal(got.view(np.uint32), outs[1].host().view(np.uint32)), what + ": second launch into the same workspace differs"
    for yb in outs:
        assert yb.others_untouched(), what + ": wrote outside its channel slice"
    want = p["pre"]
    if act:
        want = ref.lrelu(want, SLOPE) if p["z"] is None else ref.dact(want, p["z"], SLOPE)
    per_channel(got, want, what, f"igemm {op}")
    # the six configurations agree to the bit at equal s_eff (module docstring); a view changes staging / reduce path, not the order
    first = STASH.setdefault((op, name, act, s_eff), (what, got.tobytes()))
    assert first[1] == got.tobytes(), f"{what}: bits differ from [{first[0]}]"


CFGS = [1, 2, 3, 4, 5, 6]
SPLITS = [1, 3, 5, 8]      # 3 = tail loop only, 5 = one group of four + tail, 8 = two groups; each clamped by the chunk count


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("act", [0, 1], ids=["none", "lrelu"])
@pytest.mark.parametrize("name", list(CONV))
def test_conv_fwd_forced_plans(F, lib, name, act, cfg, split):
    run_forced(F, lib, "conv_fwd", name, cfg, split, act)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("act", [0, 1], ids=["plain", "dact"])
@pytest.mark.parametrize("name", [n for n in CONV if not CONV[n].get("mask")])
def test_conv_dgrad_forced_plans(F, lib, name, act, cfg, split):
    run_forced(F, lib, "conv_dgrad", name, cfg, split, act)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("act", [0, 1], ids=["none", "lrelu"])
@pytest.mark.parametrize("name", list(DECONV))
def test_deconv_fwd_forced_plans(F, lib, name, act, cfg, split):
    run_forced(F, lib, "deconv_fwd", name, cfg, split, act)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("act", [0, 1], ids=["plain", "dact"])
@pytest.mark.parametrize("name", list(DECONV))
def test_deconv_dgrad_forced_plans(F, lib, name, act, cfg, split):
    run_forced(F, lib, "deconv_dgrad", name, cfg, split, act)


VIEW_CASES = [(op, name, view) for op, name in (("conv_fwd", "c40k200_3x3"), ("conv_dgrad", "c40k200_3x3"), ("conv_fwd", "c37k70_5x5s2"),
                                                ("conv_dgrad", "c37k70_5x5s2"), ("deconv_fwd", "c48k100"), ("deconv_dgrad", "c48k100"))
              for view in ("in_slice", "in_odd", "out_odd", "z_odd") if not (view == "z_odd" and op.endswith("fwd"))]      # a forward has no xact


@pytest.mark.parametrize("plan", [(2, 5), (5, 1)], ids=["64x192_split5", "128x192w8_unsplit"])
@pytest.mark.parametrize("case", VIEW_CASES, ids=lambda c: "-".join(c))
def test_pitched_views(F, lib, case, plan):
    """operands and results as channel slices of wider buffers: pitches that keep / rule out the 16-byte staging and reduce paths"""
    op, name, view = case
    run_forced(F, lib, op, name, plan[0], plan[1], 1, view)


# ---- first layer (3-channel input, 8 taps x 4 channels per chunk) -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def first_layer(K):
    from spatiotemporalentropymodel_amd import functional as F
    B, H, W, R = 1, 17, 23, 5
    s = spread(K)
    x = rnd((B, 3, H, W), 11, 0, 1)
    w = (rnd((K, 3, R, R), 12) / np.sqrt(75)).astype(np.float32) * s[:, None, None, None]
    b = rnd((K,), 13) * s
    x4 = np.concatenate([x, np.zeros((B, 1, H, W), np.float32)], axis=1)
    return dict(B=B, H=H, W=W, R=R, K=K, x=x, w=w, b=b, x4=Buf(x4.shape, src=x4), wp=F.pack_weight(dev(w), F.PACK_CONV_FWD_C4), bias=dev(b),
                pre=ref.conv2d_fwd(x, w, b, 2, 2))


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("K", [64, 192])
def test_first_layer_forced_tiles(F, lib, K, cfg):
    """stem_conv2d_fwd_c4 under every tile; it never splits (no workspace argument): a forced igemm_split is ignored by design"""
    p = first_layer(K)
    oh, ow = ref.conv_out_hw(p["H"], p["W"], 5, 5, 2, 2)
    yb = Buf((p["B"], K, oh, ow), K + 3, 1)
    with F.tuning(igemm_cfg=cfg, igemm_split=5):
        rc = lib.stem_conv2d_fwd_c4(p["x4"].ptr, p["wp"].data_ptr(), p["bias"].data_ptr(), yb.ptr, yb.ld, p["B"], p["H"], p["W"], K, 5, 5, 2, 2, F._stream())
        assert rc == 0, lib.stem_last_error()
        assert (lib.stem_tuning_get(b"igemm_ran_cfg"), lib.stem_tuning_get(b"igemm_ran_split")) == (cfg, 1)
    torch.cuda.synchronize()
    got = yb.host()
    assert yb.others_untouched()
    per_channel(got, p["pre"], f"first layer K{K} cfg {cfg}", "igemm first layer (c4)")
    first = STASH.setdefault(("c4", K), (cfg, got.tobytes()))
    assert first[1] == got.tobytes(), f"first layer K{K}: cfg {cfg} differs in bits from cfg {first[0]}"


# ---- GDN / IGDN / denominator ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gdn_operands(C):
    beta = np.sqrt(1 + 0.2 * rnd((C,), 32) + 2.0 ** -36).astype(np.float32)
    gamma = np.sqrt(0.1 * np.eye(C) + 0.02 * np.abs(rnd((C, C), 33)) + 2.0 ** -36).astype(np.float32)
    gamma[1, :3] = 0.0                 # below 2^-18: clamped, effective value exactly 0
    gamma[2, 4] = 2.0 ** -19
    gamma[C - 1, C - 2] = 1e-7
    beta[3] = 0.0                      # below its bound
    beta[C - 1] = 5e-4
    return beta, gamma


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("inverse", [0, 1, 2], ids=["gdn", "igdn", "norm"])
@pytest.mark.parametrize("C", [64, 192, 70])
def test_gdn_forced_tiles(F, lib, C, inverse, cfg):
    """stem_gdn_fwd (x^2 and the reparametrised gamma staged by the kernel); C = 70 runs the scalar-staging GDN kernel"""
    B, H, W = 2, 9, 11
    x = rnd((B, C, H, W), 31, -3, 3)
    beta, gamma = gdn_operands(C)
    xb, yb, bt, gm = Buf(x.shape, src=x), Buf(x.shape), dev(beta), dev(gamma)
    with F.tuning(igemm_cfg=cfg, igemm_split=3):
        rc = lib.stem_gdn_fwd(xb.ptr, xb.ld, bt.data_ptr(), gm.data_ptr(), yb.ptr, yb.ld, B, H, W, C, inverse, 1e-6, F._stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.stem_last_error()
        assert (lib.stem_tuning_get(b"igemm_ran_cfg"), lib.stem_tuning_get(b"igemm_ran_split")) == (cfg, 1)      # the GDN epilogues never split
    got = yb.host()
    per_channel(got, ref.gdn_fwd(x, beta, gamma, inverse), f"gdn C{C} inverse {inverse} cfg {cfg}", "igemm gdn")
    first = STASH.setdefault(("gdn", C, inverse), (cfg, got.tobytes()))
    assert first[1] == got.tobytes(), f"gdn C{C} inverse {inverse}: cfg {cfg} differs in bits from cfg {first[0]}"


FUSED = ("conv", "c4", "deconv")


@functools.lru_cache(maxsize=None)
def fused_problem(entry, N):
    from spatiotemporalentropymodel_amd import functional as F
    s = spread(N)
    b = rnd((N,), 43) * s
    if entry == "conv":
        g = dict(B=2, C=40, H=9, W=11, R=3, st=1, pad=1, opad=0)
        x = rnd((2, 40, 9, 11), 41)
        w = (rnd((N, 40, 3, 3), 42) / np.sqrt(360)).astype(np.float32) * s[:, None, None, None]
        v, wp = ref.conv2d_fwd(x, w, b, 1, 1), F.pack_weight(dev(w), F.PACK_CONV_FWD)
    elif entry == "c4":
        g = dict(B=1, C=4, H=17, W=23, R=5, st=2, pad=2, opad=0)
        x3 = rnd((1, 3, 17, 23), 41, 0, 1)
        w = (rnd((N, 3, 5, 5), 42) / np.sqrt(75)).astype(np.float32) * s[:, None, None, None]
        v, wp = ref.conv2d_fwd(x3, w, b, 2, 2), F.pack_weight(dev(w), F.PACK_CONV_FWD_C4)
        x = np.concatenate([x3, np.zeros((1, 1, 17, 23), np.float32)], axis=1)
    else:
        g = dict(B=2, C=48, H=5, W=7, R=5, st=2, pad=2, opad=1)
        x = rnd((2, 48, 5, 7), 41)
        w = (rnd((48, N, 5, 5), 42) / np.sqrt(48 * 25 / 4)).astype(np.float32) * s[None, :, None, None]
        v, wp = ref.deconv2d_fwd(x, w, b, 2, 2, 1), F.pack_weight(dev(w), F.PACK_DECONV_FWD)
    beta, gamma = gdn_operands(N)
    return dict(g, x=x, wp=wp, bias=dev(b), beta=beta, gamma=gamma, dbeta=dev(beta), dgamma=dev(gamma), v=v)


def call_fused(F, lib, entry, p, N, xb, yb, inverse):
    a = (p["wp"].data_ptr(), p["bias"].data_ptr(), p["dbeta"].data_ptr(), p["dgamma"].data_ptr(), yb.ptr, yb.ld, p["B"], p["H"], p["W"])
    if entry == "conv":
        return lib.stem_conv2d_gdn_fwd(xb.ptr, xb.ld, *a, p["C"], N, p["R"], p["R"], p["st"], p["pad"], inverse, 1e-6, F._stream())
    if entry == "c4":
        return lib.stem_conv2d_fwd_c4_gdn(xb.ptr, *a, N, p["R"], p["R"], p["st"], p["pad"], inverse, 1e-6, F._stream())
    return lib.stem_deconv2d_gdn_fwd(xb.ptr, xb.ld, *a, p["C"], N, p["R"], p["R"], p["st"], p["pad"], p["opad"], inverse, 1e-6, F._stream())


@pytest.mark.parametrize("fuse_cfg", [2, 5])
@pytest.mark.parametrize("inverse", [0, 1], ids=["gdn", "igdn"])
@pytest.mark.parametrize("N", [64, 128, 192])
@pytest.mark.parametrize("entry", FUSED)
def test_fused_gdn_forced_tiles(F, lib, entry, N, inverse, fuse_cfg):
    """the three conv + GDN entry points on both 192-wide tiles; igemm_cfg (a 64x64 tile here) and igemm_split are ignored"""
    p = fused_problem(entry, N)
    xb, yb = Buf(p["x"].shape, src=p["x"]), Buf(p["v"].shape, N + 4, 4)
    with F.tuning(igemm_fuse_cfg=fuse_cfg, igemm_cfg=4, igemm_split=3):
        rc = call_fused(F, lib, entry, p, N, xb, yb, inverse)
        torch.cuda.synchronize()
        assert rc == 0, lib.stem_last_error()
        assert (lib.stem_tuning_get(b"igemm_ran_cfg"), lib.stem_tuning_get(b"igemm_ran_split")) == (fuse_cfg, 1)
    got = yb.host()
    assert yb.others_untouched()
    n = ref.gdn_norm(p["v"], p["beta"], p["gamma"])
    want = p["v"] * np.sqrt(n) if inverse else p["v"] / np.sqrt(n)
    per_channel(got, want, f"fused {entry} N{N} inverse {inverse} tile {fuse_cfg}", "igemm fused gdn")
    first = STASH.setdefault(("fused", entry, N, inverse), (fuse_cfg, got.tobytes()))
    assert first[1] == got.tobytes(), f"fused {entry} N{N}: tile {fuse_cfg} differs in bits from tile {first[0]}"


@pytest.mark.parametrize("entry", ["conv", "deconv"])
def test_fused_gdn_refuses_pitches_without_vector_path(F, lib, entry):
    """the fused kernels exist with 16-byte staging only: an input pitch that is no multiple of 4 is an error, nothing runs"""
    p = fused_problem(entry, 64)
    xb, yb = Buf(p["x"].shape, p["C"] + 1, 0, src=p["x"]), Buf(p["v"].shape)
    rc = call_fused(F, lib, entry, p, 64, xb, yb, 0)
    torch.cuda.synchronize()
    assert rc != 0 and b"fused GDN needs 16-byte aligned" in lib.stem_last_error(), lib.stem_last_error()
    assert bool((yb.buf == SENT).all().item())


# ---- weight gradients --------------------------------------------------------------------------------------------------------
WGRAD = {  # pixels of the loop grid: 156 / 156 / 140 / 140 / 140 -> 5 chunks of 32
    "conv_c40k72_3x3s1": dict(B=1, C=40, H=13, W=12, K=72, R=3, st=1, pad=1),                      # vector staging, db from the fused column sums
    "conv_c40k72_5x5s2": dict(B=1, C=40, H=25, W=23, K=72, R=5, st=2, pad=2),
    "conv_c37k70_5x5s2": dict(B=4, C=37, H=13, W=10, K=70, R=5, st=2, pad=2),                      # scalar staging, db from the separate pass
    "deconv_c48k100": dict(B=4, C=48, H=5, W=7, K=100, R=5, st=2, pad=2, opad=1, deconv=True),     # vector
    "deconv_c37k70": dict(B=4, C=37, H=5, W=7, K=70, R=5, st=2, pad=2, opad=1, deconv=True),       # scalar staging, scalar column sums
}
WG_CFGS = [1, 2, 3, 4, 5]
WG_SPLITS = [1, 2, 5]


@functools.lru_cache(maxsize=None)
def wgrad_problem(name):
    g = dict(WGRAD[name])
    B, C, H, W, K, R, st, pad = (g[k] for k in ("B", "C", "H", "W", "K", "R", "st", "pad"))
    deconv, opad = g.get("deconv", False), g.get("opad", 0)
    oh, ow = ref.deconv_out_hw(H, W, R, R, st, pad, opad) if deconv else ref.conv_out_hw(H, W, R, R, st, pad)
    x = rnd((B, C, H, W), 51)
    dy = rnd((B, K, oh, ow), 52) * spread(K)[None, :, None, None]
    dw = ref.deconv2d_dw(x, dy, R, R, st, pad) if deconv else ref.conv2d_dw(x, dy, R, R, st, pad)
    npix = B * H * W if deconv else B * oh * ow
    return dict(g, deconv=deconv, opad=opad, x=x, dy=dy, dw=dw, db=ref.bias_grad(dy), l1=np.abs(dy.astype(np.float64)).sum(axis=(0, 2, 3)),
                nchunks=cdiv(npix, 32))


def run_wgrad(F, lib, name, cfg, splits, slices=False, accumulate_db=False):
    p = wgrad_problem(name)
    n = p["nchunks"]
    assert cdiv(n, cdiv(n, splits)) == splits, (name, n, splits)
    C, K, R, st, pad = p["C"], p["K"], p["R"], p["st"], p["pad"]
    xb = Buf(p["x"].shape, C + 8, 4, src=p["x"]) if slices else Buf(p["x"].shape, src=p["x"])
    dyb = Buf(p["dy"].shape, K + 12, 8, src=p["dy"]) if slices else Buf(p["dy"].shape, src=p["dy"])
    db0 = rnd((K,), 53) * spread(K)
    kw = dict(db_out=dev(db0), accumulate_db=True) if accumulate_db else {}
    what = f"wgrad {name} cfg {cfg} splits {splits} slices {slices} accumulate_db {accumulate_db}"
    with F.tuning(wgrad_cfg=cfg):
        if p["deconv"]:
            dw, db = F.deconv2d_wgrad(xb.nchw(), dyb.nchw(), K, R, R, st, pad, p["opad"], splits=splits, **kw)
        else:
            dw, db = F.conv2d_wgrad(xb.nchw(), dyb.nchw(), K, R, R, st, pad, splits=splits, **kw)
        torch.cuda.synchronize()
        assert lib.stem_tuning_get(b"wgrad_ran_cfg") == cfg, (what, lib.stem_tuning_get(b"wgrad_ran_cfg"))
    per_channel(dw.cpu().numpy(), p["dw"], what + " dw", "wgrad dw", axis=1 if p["deconv"] else 0)
    want_db = p["db"] + (db0.astype(np.float64) if accumulate_db else 0.0)
    per_sum(db.cpu().numpy(), want_db, p["l1"] + (np.abs(db0) if accumulate_db else 0.0), what + " db", "wgrad db")


@pytest.mark.parametrize("splits", WG_SPLITS)
@pytest.mark.parametrize("cfg", WG_CFGS)
@pytest.mark.parametrize("name", list(WGRAD))
def test_wgrad_forced_plans(F, lib, name, cfg, splits):
    run_wgrad(F, lib, name, cfg, splits)


@pytest.mark.parametrize("name", ["conv_c40k72_3x3s1", "deconv_c48k100"])
def test_wgrad_accumulate_db_and_channel_slices(F, lib, name):
    run_wgrad(F, lib, name, 2, 2, accumulate_db=True)
    run_wgrad(F, lib, name, 5, 5, slices=True)


@pytest.mark.parametrize("splits", [None, 2])
def test_wgrad_first_layer_folded_taps(F, lib, splits):
    """3-channel input as a 4-channel NHWC image: taps folded into the tile's N axis, one tile of its own (reported as 4 = 64x64)
    whatever wgrad_cfg says; the planner's own split count (None) and a forced one"""
    B, H, W, K, R = 1, 17, 23, 64, 5
    x = rnd((B, 3, H, W), 61, 0, 1)
    x4 = np.concatenate([x, np.zeros((B, 1, H, W), np.float32)], axis=1)
    dy = rnd((B, K, 9, 12), 62) * spread(K)[None, :, None, None]
    xb, dyb = Buf(x4.shape, src=x4), Buf(dy.shape, src=dy)
    with F.tuning(wgrad_cfg=1):
        dw, db = F.conv2d_wgrad(xb.nchw(), dyb.nchw(), K, R, R, 2, 2, splits=splits)
        torch.cuda.synchronize()
        assert lib.stem_tuning_get(b"wgrad_ran_cfg") == 4
    dw = dw.cpu().numpy()
    assert dw.shape == (K, 4, R, R) and not dw[:, 3].any()
    per_channel(dw[:, :3], ref.conv2d_dw(x, dy, R, R, 2, 2), f"folded-tap dw splits {splits}", "wgrad dw (folded taps)", axis=0)
    per_sum(db.cpu().numpy(), ref.bias_grad(dy), np.abs(dy.astype(np.float64)).sum(axis=(0, 2, 3)), "folded-tap db", "wgrad db")


@pytest.mark.parametrize("cfg", WG_CFGS)
@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("C", [64, 128, 192])
def test_gdn_bwd_forced_wgrad_tiles(F, lib, C, inverse, cfg):
    """F.gdn_bwd: its gamma gradient is the weight-gradient kernel with the squared gathered operand (STEM_WGRAD_SQUARE_G)"""
    B, H, W = 2, 9, 11
    x, dy = rnd((B, C, H, W), 71, -3, 3), rnd((B, C, H, W), 72)
    beta, gamma = gdn_operands(C)
    xb, dyb = Buf(x.shape, src=x), Buf(dy.shape, src=dy)
    with F.tuning(wgrad_cfg=cfg):
        dx, dbeta, dgamma = F.gdn_bwd(xb.nchw(), dyb.nchw(), dev(beta), dev(gamma), inverse=inverse)
        torch.cuda.synchronize()
        assert lib.stem_tuning_get(b"wgrad_ran_cfg") == cfg
    rx, rb, rg = ref.gdn_bwd(x, dy, beta, gamma, inverse=inverse)
    what = f"gdn_bwd C{C} inverse {inverse} wgrad cfg {cfg}"
    per_channel(dx.cpu().numpy(), rx, what + " dx", "gdn_bwd dx")
    per_channel(dgamma.cpu().numpy(), rg, what + " dgamma", "gdn_bwd dgamma", axis=0)
    n = ref.gdn_norm(x, beta, gamma)
    gterm = np.abs(0.5 * dy * x / np.sqrt(n) if inverse else 0.5 * dy * x / (n * np.sqrt(n)))
    bb = np.sqrt(float(np.float32(1e-6)) + ref.PEDESTAL)
    per_sum(dbeta.cpu().numpy(), rb, 2.0 * np.maximum(beta.astype(np.float64), bb) * gterm.sum(axis=(0, 2, 3)), what + " dbeta", "gdn_bwd dbeta")


def test_tuning_drops_the_workspace_size_cache(F, lib):
    """a split forced AFTER a geometry's first call through functional.py still gets its workspace (and runs split)"""
    p = problem("conv_fwd", "c40k200_3x3")
    B, H, W, C, K, R, S, st, pad, _ = p["dims"]
    xb = Buf(p["inp"].shape, src=p["inp"])
    F.conv2d_fwd(xb.nchw(), p["wp"], p["bias"], K, R, S, st, pad)
    with F.tuning(igemm_cfg=4, igemm_split=5):
        y = F.conv2d_fwd(xb.nchw(), p["wp"], p["bias"], K, R, S, st, pad)
        torch.cuda.synchronize()
        assert (lib.stem_tuning_get(b"igemm_ran_cfg"), lib.stem_tuning_get(b"igemm_ran_split")) == (4, s_eff_of(p, 5))
    per_channel(y.cpu().numpy(), p["pre"], "forced split after an unforced call", "igemm conv_fwd")
    assert lib.stem_tuning_get(b"igemm_cfg") == 0 and lib.stem_tuning_get(b"igemm_split") == 0
