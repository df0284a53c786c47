"""Shapes, forms and plans of three fp16 families, with the host arithmetic of their launches restated in Python:
  * the 192-column kernel conv_f16x3_kernel<BM, DEPTH, MS> behind stem_conv2d_f16x3_fwd / stem_conv2d_f16x3_fwd_act,
  * the four-phase transposed form conv_f16x3_gen_kernel<GBM, 16, true> behind stem_tconv2d_f16x3_fwd (both csrc/conv_f16x3.hip),
  * the first-layer kernel c4gdn_f16x3_kernel<NB> (csrc/c4gdn_f16x3.hip).
Shared by tests/test_hip_f16x3_col_forms.py, tests/test_hip_tconv_forms.py, tests/test_hip_c4gdn_forms.py (GPU) and
tests/test_fx3_col_plan_abi.py (CPU); nothing here touches the library.

192-column kernel: a launch walks n = (C / 32) * R * S chunks (slab outer, taps inner), in pairs with a tail; the prologue loads
NST - 1 + 2 chunks (NST = LDS stages = 2 | 3), clamped to the last one, and the stage rotation of the three-stage loops is mod 3 --
so n = 1 .. 7 are seven different walks.  The grid is cdiv(M, BM) workgroups, re-ordered over the 8 XCDs when there are >= 16.

Four-phase form: phase p = 2 py + px of an R x R, stride-2, padding R / 2 layer is a stride-1 convolution of the coarse grid with
cnt(py) * cnt(px) taps (tconv_axis), nch[p] = (C / 32) * taps chunks; one chunks-per-workgroup number cps for the launch, clamped
per phase, nsplit[p] = cdiv(nch[p], min(cps, nch[p])); only the phases that split own slabs in the workspace.
"""
import numpy as np

CNT_BYTES = 65536          # arrival counters in front of the split-K slabs (kGenCntBytes)
GBN = 128                  # output channels per workgroup of the general kernel
BN = 192                   # ... of the 192-column kernel
UNSPLIT_CPS = 1 << 30      # "tconv_ran_cps" after the second planning pass


def cdiv(a, b):
    return -(-a // b)


def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


# ---- the 192-column kernel ---------------------------------------------------------------------------------------------------
COL_FORMS = {  # name -> (selectors, (fx3_col_ran_tile, fx3_col_ran_depth, fx3_col_ran_mfma))
    f"{bm}/{d}/{ms}": (dict(fx3_tile=bm, fx3_depth=d, fx3_mfma=ms), (bm, d, ms)) for bm in (64, 128) for d, ms in ((2, 32), (3, 32), (3, 16))
}


def col_instantiation(tile, depth, mfma):
    """(BM, DEPTH, MS) that runs under forced fx3_tile, fx3_depth, fx3_mfma: the 16-row MFMA shape exists for the three-stage loop
    only (`m16 = depth == 3 && ...`), so fx3_mfma = 16 with fx3_depth = 2 runs MS = 32"""
    assert tile in (64, 128) and depth in (2, 3) and mfma in (16, 32)
    return tile, depth, 16 if depth == 3 and mfma == 16 else 32


COL_SHAPES = {  # name -> (B, C, H, W, N, R, S, stride, pad)
    "n1_xcd_remap": (2, 32, 25, 44, 33, 1, 1, 1, 0),       # one chunk; M = 2200: 35 / 18 workgroups (>= 16, not a multiple of 8); N = 33
    "n2_m_below_64": (1, 64, 5, 9, 96, 1, 1, 1, 0),        # two chunks; M = 45; N = 96: the second wavefront column is all but dead
    "n3_1x3_pad0": (2, 32, 7, 13, 100, 1, 3, 1, 0),        # three chunks; M = 154: a tail on both tiles, tiles straddle rows and images
    "n4_stride3": (2, 128, 20, 23, 64, 1, 1, 3, 0),        # four chunks; stride 3; M = 112; N = 64: second wavefront column dead
    "n5_1x5_pad3": (1, 32, 6, 10, 192, 1, 5, 1, 3),        # five chunks; pad 3 > R / 2 and > S / 2: whole output rows outside the image
    "n6_1x3_stride2": (3, 64, 9, 14, 96, 1, 3, 2, 1),      # six chunks; stride 2, pad 1 > R / 2; M = 126
    "n7_1x7": (2, 32, 4, 20, 64, 1, 7, 1, 3),              # seven chunks; M = 400
    "3x3_c64": (2, 64, 9, 11, 96, 3, 3, 1, 1),             # 18 chunks; its input-gradient role has the same geometry
    "5x5_s2_192": (2, 192, 20, 28, 192, 5, 5, 2, 2),       # 150 chunks: the analysis transform's layer at 20 x 28
}
COL_RESID = ("n2_m_below_64", "n3_1x3_pad0", "n4_stride3", "3x3_c64", "5x5_s2_192")     # every output has at least 9 / 25 of its taps inside the image
COL_GDN = ("n1_xcd_remap", "n3_1x3_pad0", "n5_1x5_pad3", "3x3_c64", "5x5_s2_192")       # N = 33, 100, 192, 96, 192
COL_ACT = ("n2_m_below_64", "n4_stride3", "n6_1x3_stride2", "n7_1x7", "3x3_c64")


def col_chunks(C, R, S):
    return (C // 32) * R * S


def col_grid(B, C, H, W, N, R, S, stride, pad, bm):
    OH, OW = out_hw(H, W, R, S, stride, pad)
    return cdiv(B * OH * OW, bm)


def xcd_tile(bx, nb):
    """pixel tile of workgroup bx in a grid of nb (conv_f16x3_kernel's XCD-aware order); identity below 16 workgroups"""
    if nb < 16:
        return bx
    qq, rr, xcd, idx = nb >> 3, nb & 7, bx & 7, bx >> 3
    return (xcd * (qq + 1) if xcd < rr else rr * (qq + 1) + (xcd - rr) * qq) + idx


# ---- the four-phase transposed form ------------------------------------------------------------------------------------------
TCONV_SHAPES = {  # name -> (B, C, H, W, N, R, odd rows, odd columns): coarse grid H x W, fine grid (2H - odd) x (2W - odd)
    "c32_r3_n96": (2, 32, 5, 7, 96, 3, 0, 0),              # M = 70: ragged on both tiles; chunks 1 / 2 / 2 / 4
    "c64_r5_n132_odd_rows": (1, 64, 6, 9, 132, 5, 1, 0),   # M = 54 < 64; N % 32 != 0: no planes; second N tile 4 columns wide
    "c96_r5_n160_odd_cols": (3, 96, 4, 7, 160, 5, 0, 1),   # M = 84; chunks 27 / 18 / 18 / 12
    "c64_r3_n160_odd_both": (2, 64, 9, 8, 160, 3, 1, 1),   # M = 144 = 128 + 16 = 2 * 64 + 16; chunks 2 / 4 / 4 / 8
    "c32_r5_n96": (2, 32, 6, 6, 96, 5, 0, 0),              # M = 72; chunks 9 / 6 / 6 / 4
}
TCONV_TILES = (64, 128)


def tconv_axis(R, pad, par):
    """(taps of this parity, offset of the first one on the coarse grid, largest r): f16x3_layout.h"""
    rmin = (par + pad) & 1
    cnt = (R - 1 - rmin) // 2 + 1 if rmin < R else 0
    rmax = rmin + 2 * (cnt - 1)
    return cnt, (par + pad - rmax) // 2, rmax


def tconv_taps(R):
    """taps of phase p = 2 py + px"""
    return [tconv_axis(R, R // 2, p >> 1)[0] * tconv_axis(R, R // 2, p & 1)[0] for p in range(4)]


def tconv_nch(C, R):
    return [(C // 32) * t for t in tconv_taps(R)]


def tconv_plan(C, R, split=0, cps=0, room=True):
    """(cps, [nsplit of phase 0..3]) of a launch under forced fx3_split = split or tconv_cps = cps (fx3_split wins); room = False:
    the workspace is null or too small for the plan -> the second pass, unsplit"""
    nch = tconv_nch(C, R)
    maxc = max(nch)
    assert split > 0 or cps > 0, "the planner's own choice is a performance number and is not restated"
    c = cdiv(maxc, min(split, maxc)) if split > 0 else cps
    ns = [cdiv(n, min(c, n)) for n in nch]
    if max(ns) > 1 and not room:
        c, ns = UNSPLIT_CPS, [1, 1, 1, 1]
    return c, ns


def tconv_need_bytes(B, H, W, N, ns):
    """what a plan needs of the workspace: the counters and, behind each other, the slabs of the phases that split"""
    M, ntn = B * H * W, cdiv(N, GBN)
    return CNT_BYTES + 4 * sum(n * M * ntn * GBN for n in ns if n > 1)


def tconv_room_bytes(B, H, W, N):
    """stem_tconv2d_f16x3_workspace_bytes: room for any plan of the planner (16 splits of every phase)"""
    return CNT_BYTES + 4 * 16 * B * H * W * cdiv(N, GBN) * GBN * 4


def tconv_split_list(C, R):
    """fx3_split in {1, 2, 3, 5, maxc, maxc + 7}, one per distinct per-phase split vector: maxc = one chunk per workgroup in every
    phase, maxc + 7 checks the clamp (and is dropped: its vector is maxc's)"""
    maxc = max(tconv_nch(C, R))
    seen, out = set(), []
    for s in (1, 2, 3, 5, maxc, maxc + 7):
        v = tuple(tconv_plan(C, R, split=s)[1])
        if v not in seen:
            seen.add(v)
            out.append(s)
    return out


def tconv_slots(B, H, W, N, bm):
    """slots of the output's scale record: one per workgroup of the grid's first two dimensions"""
    return 4 * cdiv(B * H * W, bm) * cdiv(N, GBN)


# ---- the first-layer kernel --------------------------------------------------------------------------------------------------
C4_SHAPES = {  # name -> (B, H, W, N, R, S, stride, pad)
    "5x5_s2_n192": (2, 21, 30, 192, 5, 5, 2, 2),           # M = 330: partial last workgroup (128 pixels each)
    "one_output_pixel": (1, 5, 5, 64, 5, 5, 1, 0),         # pad 0: OH = OW = 1
    "3x3_s1_n128": (2, 9, 11, 128, 3, 3, 1, 1),            # M = 198
    "1x1_s3_n64": (3, 10, 13, 64, 1, 1, 3, 0),             # M = 60; stride 3; one conv k-step with one live slot triple
    "3x5_s2_long_rows": (1, 6, 300, 128, 3, 5, 2, 1),      # R != S; OW = 149: rows longer than a workgroup's 128 pixels; pad 1 < S / 2
    "5x5_s3_pad0": (2, 17, 20, 192, 5, 5, 3, 0),           # stride 3, pad 0; M = 60
}
C4_WG = 128


# ---- inputs ------------------------------------------------------------------------------------------------------------------
PIX_STEPS = 17             # pixel amplitudes 2^0 .. 2^-16 of the tile's maximum


def col_resid_operands(name):
    """systematic-residual activations and weights of a 192-column shape (wg3_cases.resid: all positive, the second fp16 number of
    every element +0.45 units of the first one's last place)"""
    from wg3_cases import resid
    B, C, H, W, N, R, S, stride, pad = COL_SHAPES[name]
    return resid((B, C, H, W), 11, -3), resid((N, C, R, S), 12, -14)


def tconv_resid_operands(name):
    """the same for a four-phase shape: coarse input [B,C,H,W] and the weight read as w[c][n][r][s]"""
    from wg3_cases import resid
    B, C, H, W, N, R, oh, ow = TCONV_SHAPES[name]
    return resid((B, C, H, W), 64, -3), resid((C, N, R, R), 65, -14)


def c4_resid_operands(name):
    """the same for a first-layer shape: image [B,3,H,W] of about 1 and weights of about 1e-3, so that gamma' v^2 stays far below
    beta' and the GDN passes a relative change of the convolution output on"""
    from wg3_cases import resid
    B, H, W, N, R, S, stride, pad = C4_SHAPES[name]
    return resid((B, 3, H, W), 91, -10), resid((N, 3, R, S), 92, -20)


def pixel_steps(npix):
    """exponent k of pixel p: its inputs are the base pattern times 2^-k; every 64 pixels repeat, so that 64- and 128-pixel tiles
    (and the first-layer kernel's 128-pixel workgroups) see the same maximum"""
    return (np.arange(npix) % 64) % PIX_STEPS


def square_split_error(t2):
    """what the two fp16 numbers of a scaled square t2 >= 0 may miss: 2^-22 t2 (two 11-bit significands), or half a unit of the
    subnormal grid 2^-24 where the second number is subnormal"""
    return np.maximum(2.0 ** -22 * np.asarray(t2, np.float64), 2.0 ** -25)


def amplitude_ratio_for(rtol, scaled_max=2.0 ** 6):
    """amplitude, as a fraction of the maximum the squares are scaled by, below which the norm's relative error 2^-25 / t^2 makes
    the output's (half of it) exceed rtol; scaled_max: what that maximum becomes (2^6 .. 2^7 in the 192-column kernel)"""
    return float(np.sqrt(2.0 ** -26 / rtol) / scaled_max)
