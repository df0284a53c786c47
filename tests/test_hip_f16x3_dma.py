"""GPU: the LDS ring of csrc/conv_f16x3.hip is filled by LDS-DMA (global -> LDS, no vector registers): the smallest shapes at
which that fill can go wrong, in both kernels, under every forced plan, each launched RIGHT AFTER a launch of another shape whose
operands sit at the top of their range on every CU -- a copy that lands late, in the wrong stage or not at all then shows as an
error of the order of the result, not as the previous launch's (equal) data.

What the fill has to get right (conv_f16x3.hip, "LDS-DMA"): wavefront w copies rows 16 w .. 16 w + 15 of each activation plane,
lane l -> row l / 4, LDS slot l % 4, source piece slot ^ ((row >> 2) & 3); taps outside the image and rows m >= M take the offset
every buffer view rejects (zeros); the weight chunk is copied linearly, 1 KiB per wavefront and pass; the counted waits of the
three-stage loops (all but the youngest chunk) and the wait + barrier in front of every reuse of the ring (fused GDN, split-K
hand-over, planes pass).

192-column kernel, 5x5 / stride 2 / pad 2, N = 192, with and without the fused GDN, all six instantiations (fx3_tile 64 | 128,
fx3_depth 2 | 3, fx3_mfma 32 | 16, read back through fx3_col_ran_*):
  * C = 32, B = 1, 9 x 9 -> M = 25: one ragged tile, every output pixel has taps outside the image; 25 chunks;
  * C = 64, B = 3, 12 x 12 -> M = 108: two slabs (50 chunks), ragged for both tile sizes, tiles straddle images.
General kernel (fx3_gen_tile 64 | 128, fx3_gen_mfma 32 | 16, fx3_split 1 | 3, read back through fx3_ran_*), bias + leaky ReLU,
fp32 and planes outputs:
  * 1x1, C = 96 -> N = 160 on 2 x 7 x 7: the second N tile has 32 live columns (one wavefront column dead: copies and barriers only);
  * 3x3 and 5x5 "same", C = 64 -> N = 96, on 2 x 7 x 7 (M = 98: ragged for both tiles) and 2 x 8 x 8 (M = 128: exact);
  * the 12 live taps of the 5x5 type-A mask;
  * the 3x3 input read as channels [32, 96) of a planes tensor 32 channels wider (pixel pitch and slab offset in the copy's offsets);
  * the transposed 5x5 stride-2 face, 4 x 4 -> 8 x 8 (four phases in one launch; phases with fewer splits leave at once).

Reference: float64 convolution (+ GDN) computed here with torch on the CPU.  Gate: the one tests/test_hip_f16x3_forms.py holds
the same kernels to -- every output channel within 1e-4 of ITS OWN maximum, no floor (per_channel; planes outputs: or the grid of
their second fp16 number); output channel k of weights and bias carries the scale 2^(-20 k / (N - 1)).  The launches go through the
forced-plan drivers of the three existing form tests (double launch bit-identical, NaN-poisoned split-K slabs, sentinels around the
output's channel slice, read-back of the plan that ran).
"""
import functools

import numpy as np
import pytest
import torch

import fx3_col_cases as K
import test_hip_f16x3_col_forms as col
import test_hip_f16x3_forms as gen
import test_hip_tconv_forms as tconv
from test_hip_fp32_plans import SLOPE, dev, rnd, spread

pytestmark = pytest.mark.gpu

PEDESTAL = 2.0 ** -36
BETA_MIN = 1e-6
GEN_FORMS = [f for f in gen.FORMS if f != "img"]


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return functional


@pytest.fixture(scope="module")
def lib(F):
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def conv64(x, w, stride, pad):
    return torch.nn.functional.conv2d(t64(x), t64(w), None, stride, pad).numpy()


def gdn64(v, beta, gamma):
    """y = v / sqrt(beta' + gamma' v^2), beta' = max(beta, sqrt(beta_min + 2^-36))^2 - 2^-36, gamma' = max(gamma, 2^-18)^2 - 2^-36"""
    bp = torch.clamp(t64(beta), min=float(np.sqrt(float(np.float32(BETA_MIN)) + PEDESTAL))) ** 2 - PEDESTAL
    gp = torch.clamp(t64(gamma), min=2.0 ** -18) ** 2 - PEDESTAL
    v = t64(v)
    return (v / torch.sqrt(torch.einsum("ij,bjhw->bihw", gp, v * v) + bp[None, :, None, None])).numpy()


def with_bias(pre, b):
    return pre + np.asarray(b, np.float64)[None, :, None, None]


def lrelu64(v):
    return np.where(v > 0, v, v * SLOPE)


# ---- the launch in front of every case: operands at the top of their range, at least one workgroup on every CU ---------------
@functools.lru_cache(maxsize=None)
def poison_operands(family):
    from spatiotemporalentropymodel_amd import functional as F
    B, C, H, W, N = 1, 32, 182, 182, 192 if family == "col" else 128          # M = 33124: 259 / 518 workgroups
    x = torch.full((B, C, H, W), 3.0e4, device="cuda")
    x[:, :8] = -3.0e4
    w = torch.full((N, C, 1, 1), 2.0e3, device="cuda")
    return F.F16Planes.split(x), F.pack_weight_f16x2(w) if family == "col" else F.pack_weight_f16x2_gen(w), N


def poison(F, family):
    xp, wp, N = poison_operands(family)
    if family == "col":
        F.conv2d_f16x3_fwd(xp, wp, None, N, 1, 1, 1, 0, planes_out=True)
    else:
        F.conv2d_f16x3_gen(xp, wp, None, N, 1, 1, 1, 0, want_fp32=False, want_planes=True)


# ---- 192-column kernel -----------------------------------------------------------------------------------------------------
COL_SHAPES = {"c32_m25": (1, 32, 9, 9), "c64_m108": (3, 64, 12, 12)}


@functools.lru_cache(maxsize=None)
def col_problem(name):
    from spatiotemporalentropymodel_amd import functional as F
    B, C, H, W = COL_SHAPES[name]
    N, R, st, pad = 192, 5, 2, 2
    sn = spread(N)
    x = rnd((B, C, H, W), 101)
    w = (rnd((N, C, R, R), 102) / np.sqrt(C * R * R)).astype(np.float32) * sn[:, None, None, None]
    b = rnd((N,), 103) * sn
    beta = rnd((N,), 104, 0.5, 1.5)
    gamma = (rnd((N, N), 105, 0.0, 0.1) + 0.1 * np.eye(N, dtype=np.float32)).astype(np.float32)
    pre = with_bias(conv64(x, w, st, pad), b)
    assert pre.shape[0] * pre.shape[2] * pre.shape[3] == {"c32_m25": 25, "c64_m108": 108}[name]
    return dict(name="dma_" + name, dims=(B, H, W, C, N, R, R, st, pad), xp=F.F16Planes.split(dev(x)), wp=F.pack_weight_f16x2(dev(w)), bias=dev(b),
                beta=dev(beta), gp=F.pack_gdn_gamma_f16x2(dev(gamma)), conv=pre, gdn=gdn64(pre, beta, gamma))


@pytest.mark.parametrize("fused", [False, True], ids=["conv", "gdn"])
@pytest.mark.parametrize("form", list(K.COL_FORMS))
@pytest.mark.parametrize("name", list(COL_SHAPES))
def test_col_kernel_after_another_shape(F, lib, name, form, fused):
    p = col_problem(name)
    epi = dict(beta=p["beta"], gp=p["gp"]) if fused else {}
    want = p["gdn"] if fused else p["conv"]
    for out in ("fp32", "planes"):
        poison(F, "col")
        col.run_forced(F, lib, p, form, "fwd", want, f"{name} {'gdn' if fused else 'conv'} {out}", bias=p["bias"], out=out, **epi)


# ---- general kernel ----------------------------------------------------------------------------------------------------------
GEN_SHAPES = {  # name -> (B, C, H, W, N, R, taps, channel view)
    "1x1_c96_n160": (2, 96, 7, 7, 160, 1, 0, False),
    "3x3_m98": (2, 64, 7, 7, 96, 3, 0, False),
    "3x3_m128": (2, 64, 8, 8, 96, 3, 0, False),
    "5x5_m98": (2, 64, 7, 7, 96, 5, 0, False),
    "5x5_m128": (2, 64, 8, 8, 96, 5, 0, False),
    "5x5_mask_a_12": (2, 64, 7, 7, 96, 5, 12, False),
    "3x3_channel_view": (2, 64, 7, 7, 96, 3, 0, True),
}


@functools.lru_cache(maxsize=None)
def gen_problem(name):
    from spatiotemporalentropymodel_amd import functional as F
    B, C, H, W, N, R, taps, view = GEN_SHAPES[name]
    sn = spread(N)
    x = rnd((B, C, H, W), 111)
    w = (rnd((N, C, R, R), 112) / np.sqrt(C * (taps or R * R))).astype(np.float32) * sn[:, None, None, None]
    if taps:
        mask = np.zeros((R, R), np.float32)
        mask.reshape(-1)[:taps] = 1.0                      # type A: the taps before the centre in raster order
        assert taps == (R // 2) * R + R // 2
        w = (w * mask).astype(np.float32)
    b = rnd((N,), 113) * sn
    if view:                                              # channels [32, 32 + C) of a tensor 32 channels wider; the unread ones set its scale
        big = F.F16Planes.split(dev(np.concatenate([3.0 * rnd((B, 32, H, W), 114), x], axis=1)))
        xp = big.channels(32, 32 + C)
        assert xp.pix_bytes == (C // 32 + 1) * 128
    else:
        xp = F.F16Planes.split(dev(x))
    return dict(name="dma_" + name, dims=(B, H, W, C, N, R), taps=taps, xp=xp, wp=F.pack_weight_f16x2_gen(dev(w.copy()), taps=taps), bias=dev(b),
                want=lrelu64(with_bias(conv64(x, w, 1, R // 2), b)))


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("form", GEN_FORMS)
@pytest.mark.parametrize("name", list(GEN_SHAPES))
def test_gen_kernel_after_another_shape(F, lib, name, form, s):
    p = gen_problem(name)
    poison(F, "gen")
    gen.run_forced(F, lib, p, form, s, gen.EPI_LRELU, p["want"], name, bias=p["bias"], planes=True)


@functools.lru_cache(maxsize=None)
def tconv_problem():
    """the forward of ConvTranspose2d(64, 96, 5, stride 2, padding 2, output_padding 1) on 2 x 4 x 4 -> 8 x 8"""
    from spatiotemporalentropymodel_amd import functional as F
    B, C, H, W, N, R = 2, 64, 4, 4, 96, 5
    sn = spread(N)
    x = rnd((B, C, H, W), 121)
    w = (rnd((C, N, R, R), 122) / np.sqrt(C * R * R / 4)).astype(np.float32) * sn[None, :, None, None]
    b = rnd((N,), 123) * sn
    pre = torch.nn.functional.conv_transpose2d(t64(x), t64(w), None, 2, R // 2, 1).numpy()
    assert pre.shape == (B, N, 2 * H, 2 * W)
    return dict(name="dma_tconv_5x5", dims=(B, H, W, C, N, R, 2 * H, 2 * W), xp=F.F16Planes.split(dev(x)), wp=F.pack_weight_f16x2_tconv(dev(w)),
                bias=dev(b), want=lrelu64(with_bias(pre, b)))


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("tile", K.TCONV_TILES)
def test_transposed_face_after_another_shape(F, lib, tile, s):
    p = tconv_problem()
    poison(F, "gen")
    tconv.run_forced(F, lib, p, tile, gen.EPI_LRELU, p["want"], "5x5 face 4x4 -> 8x8", split=s, bias=p["bias"], out="planes")
