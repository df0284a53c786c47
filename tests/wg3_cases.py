"""Shapes, plans and inputs of the fp16 weight-gradient family (csrc/wgrad_f16x3.hip: the per-tap wgrad_f16x3_kernel, the
filter-row wgrad_f16x3_row_kernel<1|3|5>, the strided entry), with the host arithmetic of a launch restated in Python.
Shared by tests/test_hip_wg3_forms.py (GPU) and tests/test_wg3_plan_abi.py (CPU); nothing here touches the library.

A launch contracts over M = B * OH * OW output pixels in chunks of 16; split z of `splits` owns the chunks [z * cps, min((z + 1) *
cps, nchunks)) with cps = cdiv(nchunks, splits) and writes slab [z][tap][K][C] (and row z of bias_part [splits][K]).  The row
form (one workgroup = 128 k x 64 c x all S taps of one filter row) is launched one-dimensionally on cdiv(tiles * R * splits, 8) * 8
workgroups, dealt to the 8 XCDs; the surplus workgroups return at once.
"""
import numpy as np

PX = 16                        # pixels per chunk
TK = TC = 128                  # per-tap workgroup tile
RT_K, RT_C = 128, 64           # filter-row workgroup tile
R_MINCHUNKS = 64               # chunks per split the row planner keeps when nothing is forced
MAXTAP = 25

# ---- shapes ------------------------------------------------------------------------------------------------------------------
ROW_SHAPES = {  # name -> (B, C, H, W, K, R): stride 1, 'same' padding, W % 16 == 0
    "3x3_ring_wraps": (2, 64, 8, 16, 96, 3),           # 16 chunks: the ring wraps, splits cross the image boundary; K = 96 masks half a wavefront's rows
    "5x5_rows_outside": (2, 96, 2, 32, 160, 5),        # H < R: filter rows 0 and 4 never meet the image; two chunks per row; half-dead c and k tiles
    "5x5_one_row": (1, 32, 1, 48, 32, 5),              # H = 1; one live wavefront of four; 3 chunks: splits of 2 + 1 and 1 + 1 + 1
    "1x1_three_k_tiles": (3, 32, 4, 16, 288, 1),       # S = 1; at split 12: 36 workgroups in a grid of 40
    "5x5_idle_workgroup": (1, 64, 2, 16, 288, 5),      # 15 workgroups in a grid of 16; two chunks
}
TAP_SHAPES = {  # name -> (B, C, H, W, K, R, S, pad): stride 1, per-tap kernel
    "one_partial_chunk": (1, 32, 3, 3, 32, 3, 3, 1),   # M = 9: all three prologue loads clamp to the same chunk
    "two_chunks": (1, 64, 4, 8, 96, 3, 3, 1),
    "33_chunks_ragged": (2, 64, 9, 29, 96, 3, 3, 1),   # M = 522; forced split 2: 17 + 16 chunks, an odd and an even loop
    "dead_wavefronts": (1, 160, 5, 7, 288, 3, 3, 1),   # 2 x 3 tiles, dead wavefronts on both axes
    "pad0_16x16_output": (2, 64, 18, 18, 96, 3, 3, 0),  # the OUTPUT is 16 x 16: must not take the row form
    "pad2_3x3": (1, 32, 6, 7, 64, 3, 3, 2),            # taps two pixels outside
    "1x5_window": (1, 32, 5, 12, 64, 1, 5, 2),
    "5x1_window": (1, 32, 5, 12, 64, 5, 1, 2),
}
STRIDED_SHAPES = {  # name -> (B, C, H, W, K, R, stride, pad); C on the fine grid H x W, K on the coarse one
    "s2_odd_fine_grid": (2, 64, 9, 11, 96, 5, 2, 2),
    "s3": (2, 64, 20, 23, 96, 5, 3, 2),
    "s4_unread_pixels": (1, 32, 13, 17, 64, 3, 4, 1),  # fine pixels that no tap reads
    "s2_two_splits": (8, 64, 16, 16, 96, 5, 2, 2),     # 32 chunks: a forced split 2 holds
    "s1_is_the_stride1_entry": (2, 64, 9, 29, 96, 3, 1, 1),
}
BENCH_LAYERS = {  # the P-frame step's layers at the bench size (geometry: tests/test_hip_fullsize.py, test_hip_f16x3.WGS_CASES)
    "TPM.2": (16, 256, 16, 16, 320, 5, 1, 2),
    "TPM.4": (16, 320, 16, 16, 384, 5, 1, 2),
    "EPM.0": (16, 1152, 16, 16, 768, 1, 1, 0),
    "HE.2": (16, 256, 16, 16, 256, 5, 2, 2),
    "HE.4": (16, 256, 8, 8, 256, 5, 2, 2),
}
ROW_SELECTORS = (0, 1, 3, 6)   # stem_tuning_set("wg3_row", .): 1 = per-tap form everywhere, 3 = 5 x 5 rows only, 6 = not the 1 x 1 layers


def cdiv(a, b):
    return -(-a // b)


def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


# ---- the planners of csrc/wgrad_f16x3.hip ----------------------------------------------------------------------------------------
def row_form(H, W, R, S, pad, sel=0):
    OH, OW = out_hw(H, W, R, S, 1, pad)
    window = R == 5 or (R == 3 and sel != 3) or (R == 1 and sel not in (3, 6))
    return sel != 1 and R == S and window and pad == R // 2 and OH == H and OW == W and OW % PX == 0


def plan_splits(B, OH, OW, C, K, T, rows=False, R=0, forced=0, minch=0):
    if rows:
        nchunks, wgs = B * OH * OW // PX, cdiv(K, RT_K) * cdiv(C, RT_C) * R
        s = forced if forced > 0 else 512 // wgs
        m = minch if minch > 0 else R_MINCHUNKS
        if forced <= 0 and s > nchunks // m:
            s = nchunks // m
        s = max(1, min(s, nchunks))
        return cdiv(nchunks, cdiv(nchunks, s))
    nchunks, tiles = cdiv(B * OH * OW, PX), cdiv(K, TK) * cdiv(C, TC) * T
    s = forced if forced > 0 else (512 + tiles // 2) // tiles
    s = max(s, 1)
    if s > nchunks // 16:                                  # at least 16 chunks per split
        s = max(nchunks // 16, 1)
    if forced <= 0 and T == 1 and s > nchunks // 32 and nchunks >= 64:      # one-tap layers: at least 32
        s = nchunks // 32
    return cdiv(nchunks, cdiv(nchunks, s))


def splits_s1(B, C, H, W, K, R, S, pad, sel=0, forced=0, minch=0):
    """stem_wgrad_f16x3_splits under wg3_row = sel, wg3_split = forced, wg3_minch = minch"""
    OH, OW = out_hw(H, W, R, S, 1, pad)
    if OH < 1 or OW < 1:
        return 0
    return plan_splits(B, OH, OW, C, K, R * S, row_form(H, W, R, S, pad, sel), R, forced, minch)


def splits_strided(B, C, H, W, K, R, S, stride, pad, forced=0):
    """stem_wgrad_f16x3_strided_splits (always the per-tap kernel; wg3_row and wg3_minch do not enter)"""
    if stride < 1:
        return 0
    OH, OW = out_hw(H, W, R, S, stride, pad)
    if OH < 1 or OW < 1:
        return 0
    return plan_splits(B, OH, OW, C, K, R * S, forced=forced)


def nchunks_of(B, OH, OW):
    return cdiv(B * OH * OW, PX)


def chunk_ranges(nchunks, splits):
    """[q_begin, q_end) of every split of a launch"""
    cps = cdiv(nchunks, splits)
    return [(z * cps, min(z * cps + cps, nchunks)) for z in range(splits)]


def row_grid(C, K, R, splits):
    """(workgroups launched, workgroups with work, idle ones, nper = workgroups per XCD) of the row form"""
    total = cdiv(K, RT_K) * cdiv(C, RT_C) * R * splits
    grid = cdiv(total, 8) * 8
    return grid, total, grid - total, grid // 8


def forced_list(splits_of):
    """wg3_split in {1, 2, 3, 5, n, n + 7} with n = the largest split count the planner grants, one per effective split;
    splits_of(forced) -> effective splits"""
    n = splits_of(1 << 20)
    seen, out = set(), []
    for s in (1, 2, 3, 5, n, n + 7):
        e = splits_of(s)
        if e not in seen:
            seen.add(e)
            out.append(s)
    return out


def row_forced_list(name):
    B, C, H, W, K, R = ROW_SHAPES[name]
    return forced_list(lambda f: splits_s1(B, C, H, W, K, R, R, R // 2, 0, f))


def tap_forced_list(name, sel=1):
    B, C, H, W, K, R, S, pad = TAP_SHAPES[name]
    return forced_list(lambda f: splits_s1(B, C, H, W, K, R, S, pad, sel, f))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
X_EXP, DY_EXP = -3, 5          # the systematic-residual operands are (m + 0.45) * 2^X_EXP and (n + 0.45) * 2^DY_EXP
RESID_LO, RESID_HI = 1024, 1100


def ints(shape, seed, pin):
    """integers in [-8, 8], element 0 pinned to `pin` = +-8 (the tensor's maximum, hence its scale, is known): both fp16 planes
    exact, the second one zero"""
    a = np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float32)
    a.reshape(-1)[0] = pin
    return a


def resid(shape, seed, exp):
    """(m + 0.45) * 2^exp, m integer in [1024, 1100]: all positive, and in the planes every element's second number is +0.45 units
    of the first one's last place -- a1 / a0 between 0.45 / 1100 and 0.45 / 1024, so each cross term a1.b0, a0.b1 carries about
    4e-4 of EVERY output, with one sign"""
    m = np.random.default_rng(seed).integers(RESID_LO, RESID_HI + 1, size=shape)
    return ((m + 0.45) * 2.0 ** exp).astype(np.float32)


def planes_of(v):
    """the two fp16 numbers of every element and the exponent e (csrc/stem_common.h: max * 2^e in [2^14, 2^15))"""
    v = np.asarray(v, np.float32)
    e = 14 - int(np.floor(np.log2(float(np.abs(v).max()))))
    s = v.astype(np.float64) * 2.0 ** e
    p0 = s.astype(np.float16)
    p1 = (s - p0.astype(np.float64)).astype(np.float16)
    return p0.astype(np.float64), p1.astype(np.float64), e
