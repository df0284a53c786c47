"""Shapes, forms and split plans of the general fp16 forward family (stem_conv2d_f16x3_gen_fwd: conv_f16x3_gen_kernel with 64- and
128-pixel tiles, the image-tile form of csrc/conv_f16x3_img.hip), with the host arithmetic of the launch restated in Python.
Shared by tests/test_hip_f16x3_forms.py (GPU) and tests/test_f16x3_plan_abi.py (CPU); nothing here touches the library.

A launch walks n = (C / 32) * T chunks (T = live taps); a forced split s runs s_eff = cdiv(n, cps) workgroups per tile with
cps = cdiv(n, min(s, n)) chunks each, split z starting at chunk q = z * cps = slab * T + tap.
"""
CNT_BYTES = 65536          # arrival counters in front of the split-K slabs (kGenCntBytes)
TS, GBN = 16, 128          # image tile edge, output channels per workgroup

SHAPES = {  # name -> (B, C, H, W, N, R, taps); taps = 0: all R*R taps
    "partial_tile_both_ways": (2, 64, 12, 12, 96, 3, 0),      # one 12x12 tile per image; wn = 1 half live; M tail of both general tiles
    "one_row_last_tile": (1, 96, 33, 16, 160, 5, 0),          # three tiles high, the third has one row; second N tile: 32 columns, wn = 1 dead
    "masked_a_column_tail": (3, 64, 16, 23, 64, 5, 12),       # T = 12 != 25; second tile 7 columns wide; N = 64: wn = 1 dead; bimg up to 2
    "masked_b_3x3": (2, 64, 12, 12, 128, 3, 5),               # T = 5: the tap walk ends mid-row
    "one_slab": (2, 32, 16, 16, 128, 3, 0),                   # s_last == s0: no second halo
    "1x1_single_chunk": (2, 32, 16, 16, 128, 1, 0),           # KS = 1; c + 1 < q_end is false in the prologue
    "1x1_n132": (2, 160, 16, 16, 132, 1, 0),                  # every chunk ends its slab; second N tile 4 columns wide; N % 32 != 0: no planes
    "2x2_tiles": (1, 64, 24, 24, 192, 3, 0),                  # four tiles, all partial on one edge; two N tiles
}
FORMS = {  # name -> (selectors, fx3_ran_form, fx3_ran_mfma)
    "gen64/32": (dict(fx3_gen_img=1, fx3_gen_tile=64, fx3_gen_mfma=32), 1, 32),
    "gen64/16": (dict(fx3_gen_img=1, fx3_gen_tile=64, fx3_gen_mfma=16), 1, 16),
    "gen128/32": (dict(fx3_gen_img=1, fx3_gen_tile=128, fx3_gen_mfma=32), 2, 32),
    "gen128/16": (dict(fx3_gen_img=1, fx3_gen_tile=128, fx3_gen_mfma=16), 2, 16),
    "img": (dict(fx3_gen_img=2, fx3_gen_tile=0), 3, 32),
}


def cdiv(a, b):
    return -(-a // b)


def live_taps(R, taps):
    return taps or R * R


def chunks(C, R, taps):
    return (C // 32) * live_taps(R, taps)


def s_eff(n, s):
    return cdiv(n, cdiv(n, min(s, n)))


def split_list(n):
    """s in {1, 2, 3, 5, n, n + 7}, one per effective split: n + 7 checks the clamp, s = n gives one chunk per workgroup"""
    seen, out = set(), []
    for s in (1, 2, 3, 5, n, n + 7):
        if s_eff(n, s) not in seen:
            seen.add(s_eff(n, s))
            out.append(s)
    return out


def q_begins(n, s):
    cps = cdiv(n, min(s, n))
    return [z * cps for z in range(s_eff(n, s))]


def img_eligible_forced(B, H, W, N, R):
    """stem_fx3_img_eligible under fx3_gen_img = 2 with no pixel tile forced, for a stride-1 "same" R x R layer"""
    tiles = cdiv(H, TS) * cdiv(W, TS)
    return R in (1, 3, 5) and H * W * 2 >= tiles * TS * TS and B * tiles * cdiv(N, GBN) <= 16384


def workspace_bytes(B, H, W, N, n, s):
    """stem_conv2d_f16x3_gen_workspace_bytes under a forced split s: room for min(s, n) slabs of M x cdiv(N, 128) * 128 floats"""
    sp = min(s, n)
    return CNT_BYTES + sp * B * H * W * cdiv(N, GBN) * GBN * 4 if sp > 1 else 0
