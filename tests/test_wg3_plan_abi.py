"""CPU: the host side of the fp16 weight-gradient family's plans (csrc/wgrad_f16x3.hip) -- the get-only read-backs of the plan
that ran ("wg3_ran_form", "wg3_ran_taps", "wg3_ran_split"), stem_wgrad_f16x3_splits / stem_wgrad_f16x3_strided_splits (host-only
functions) against the restatement of row_form and plan_splits in tests/wg3_cases.py under every selector, the case table itself
(the edges tests/test_hip_wg3_forms.py claims to reach, computed from the restatement), and a numpy emulation of the
three-product arithmetic on the systematic-residual inputs: they must make a lost cross product visible in EVERY output."""
import contextlib

import numpy as np
import pytest

import wg3_cases as W3

RAN = (b"wg3_ran_form", b"wg3_ran_taps", b"wg3_ran_split")


@pytest.fixture(scope="module")
def lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


@contextlib.contextmanager
def selectors(lib, **sel):
    old = {k: lib.stem_tuning_get(k.encode()) for k in sel}
    try:
        for k, v in sel.items():
            assert lib.stem_tuning_set(k.encode(), v) == 0, (k, v, lib.stem_last_error())
        yield
    finally:
        for k, v in old.items():
            lib.stem_tuning_set(k.encode(), v)


def test_read_backs_are_get_only(lib):
    import torch
    for name in RAN:
        before = lib.stem_tuning_get(name)
        assert before >= 0 and (before == 0 or torch.cuda.is_available()), name          # 0 until the family's first launch in this process
        assert lib.stem_tuning_set(name, before + 1) != 0 and name in lib.stem_last_error() and b"get-only" in lib.stem_last_error()
        assert lib.stem_tuning_set(name, 0) != 0 and lib.stem_tuning_get(name) == before


def s1_geometries():
    out = [(n, (B, C, H, W, K, R, R, R // 2)) for n, (B, C, H, W, K, R) in W3.ROW_SHAPES.items()]
    out += list(W3.TAP_SHAPES.items())
    out += [(n, (B, C, H, W, K, R, R, pad)) for n, (B, C, H, W, K, R, st, pad) in W3.BENCH_LAYERS.items() if st == 1]
    out += [("3x3_routing", (1, 32, 2, 16, 32, 3, 3, 1)), ("empty_output", (1, 32, 2, 2, 32, 5, 5, 0))]
    return out


@pytest.mark.parametrize("sel", W3.ROW_SELECTORS)
def test_stride1_planner_equals_the_restatement(lib, sel):
    for name, (B, C, H, W, K, R, S, pad) in s1_geometries():
        OH, OW = W3.out_hw(H, W, R, S, 1, pad)
        n = W3.nchunks_of(B, OH, OW)
        for forced in (0, 1, 2, 3, 5, 12, 16, n, n + 7):
            for minch in (0, 1, 2, 48) if forced == 0 else (0, 2):
                with selectors(lib, wg3_row=sel, wg3_split=forced, wg3_minch=minch):
                    got = int(lib.stem_wgrad_f16x3_splits(B, H, W, C, K, R, S, pad))
                want = W3.splits_s1(B, C, H, W, K, R, S, pad, sel, forced, minch)
                assert got == want, (name, sel, forced, minch, got, want)
                if OH < 1:
                    assert got == 0
                    continue
                # the cdiv round trip: every split owns at least one chunk, the last one ends on the last chunk
                rng = W3.chunk_ranges(n, got)
                assert all(b < e for b, e in rng) and rng[-1][1] == n and rng[0][0] == 0, (name, sel, forced, rng)
                if not W3.row_form(H, W, R, S, pad, sel) and got > 1:
                    assert W3.cdiv(n, got) >= 16, (name, forced, rng)                  # the per-tap clamp: at least 16 chunks per split


def test_strided_planner_equals_the_restatement(lib):
    geoms = list(W3.STRIDED_SHAPES.items()) + [(n, g) for n, g in W3.BENCH_LAYERS.items() if g[6] == 2]
    geoms += [("stride0", (1, 32, 4, 4, 32, 3, 0, 1)), ("empty", (1, 32, 2, 2, 32, 5, 2, 0))]
    for name, (B, C, H, W, K, R, st, pad) in geoms:
        for forced in (0, 1, 2, 3, 5, 40):
            for sel in (0, 1):                                      # wg3_row does not enter: the strided entry has one kernel
                with selectors(lib, wg3_row=sel, wg3_split=forced, wg3_minch=1):
                    got = int(lib.stem_wgrad_f16x3_strided_splits(B, H, W, C, K, R, R, st, pad))
                assert got == W3.splits_strided(B, C, H, W, K, R, R, st, pad, forced), (name, forced, got)
    B, C, H, W, K, R, st, pad = W3.STRIDED_SHAPES["s2_two_splits"]
    assert W3.splits_strided(B, C, H, W, K, R, R, st, pad, 2) == 2 and W3.splits_strided(B, C, H, W, K, R, R, st, pad, 3) == 2


def test_bench_layers_take_the_documented_plans():
    """the planner's own choice for the P-frame step: at most four splits for the 4096-pixel row-form layers (R_MINCHUNKS = 64),
    the one-tap rule only where the row form is switched off"""
    for name, (B, C, H, W, K, R, st, pad) in W3.BENCH_LAYERS.items():
        if st != 1:
            continue
        assert W3.row_form(H, W, R, R, pad), name
        assert W3.splits_s1(B, C, H, W, K, R, R, pad) <= 4, name
    B, C, H, W, K, R, st, pad = W3.BENCH_LAYERS["EPM.0"]
    assert W3.splits_s1(B, C, H, W, K, R, R, pad, sel=1) == 256 // 32 == 8            # nchunks / 32 (unclamped it would be 9)
    assert (512 + 54 // 2) // 54 == 9 and W3.splits_s1(B, C, H, W, K, R, R, pad, sel=1, forced=9) == 9
    assert W3.splits_s1(B, C, H, W, K, R, R, pad, sel=6) == 8 and W3.splits_s1(B, C, H, W, K, R, R, pad, sel=3) == 8


def test_selector_routing_of_the_restatement():
    five, three, one = (1, 32, 2, 16, 32, 5, 5, 2), (1, 32, 2, 16, 32, 3, 3, 1), (1, 32, 2, 16, 32, 1, 1, 0)
    form = lambda g, sel: W3.row_form(*g[2:4], *g[5:8], sel)
    assert [form(g, 0) for g in (five, three, one)] == [True, True, True]
    assert [form(g, 1) for g in (five, three, one)] == [False, False, False]
    assert [form(g, 3) for g in (five, three, one)] == [True, False, False]
    assert [form(g, 6) for g in (five, three, one)] == [True, True, False]
    for name, (B, C, H, W, K, R, S, pad) in W3.TAP_SHAPES.items():
        assert not W3.row_form(H, W, R, S, pad), name                    # whatever wg3_row says
    for name, (B, C, H, W, K, R) in W3.ROW_SHAPES.items():
        assert W3.row_form(H, W, R, R, R // 2) and C % 32 == 0 and K % 32 == 0, name
    B, C, H, W, K, R, S, pad = W3.TAP_SHAPES["pad0_16x16_output"]
    assert W3.out_hw(H, W, R, S, 1, pad) == (16, 16)


def row_split_plans():
    """(name, forced, [(q_begin, q_end)], chunks per image row, chunks per image) of every row-form case"""
    out = []
    for name, (B, C, H, W, K, R) in W3.ROW_SHAPES.items():
        n = B * H * W // W3.PX
        for f in W3.row_forced_list(name):
            s = W3.splits_s1(B, C, H, W, K, R, R, R // 2, 0, f)
            out.append((name, f, W3.chunk_ranges(n, s), W // W3.PX, H * W // W3.PX))
    return out


def test_row_cases_reach_the_short_splits_and_the_boundaries():
    plans = row_split_plans()
    lengths = {e - b for _, _, rng, _, _ in plans for b, e in rng}
    assert {1, 2, 3} <= lengths and max(lengths) >= 5, lengths            # the ring's prologue re-fetches the last chunk below 4
    assert any(len(rng) > 1 and e - b == 1 for _, _, rng, _, _ in plans for b, e in rng)
    assert any(b % per_row for _, _, rng, per_row, _ in plans for b, _ in rng[1:]), "no split starts mid image row"
    assert any(b % per_img == 0 for _, _, rng, _, per_img in plans for b, _ in rng[1:]), "no split starts on an image boundary"
    assert any(b // per_img != (e - 1) // per_img for _, _, rng, _, per_img in plans for b, e in rng), "no split crosses an image boundary"
    n = 3                                                                  # the H = 1 shape: 2 + 1 and 1 + 1 + 1
    assert W3.chunk_ranges(n, 2) == [(0, 2), (2, 3)] and W3.chunk_ranges(n, 3) == [(0, 1), (1, 2), (2, 3)]
    for name in W3.ROW_SHAPES:
        fl = W3.row_forced_list(name)
        B, C, H, W, K, R = W3.ROW_SHAPES[name]
        n = B * H * W // W3.PX
        effs = [W3.splits_s1(B, C, H, W, K, R, R, R // 2, 0, f) for f in fl]
        assert fl[0] == 1 and effs[0] == 1 and effs[-1] == n and len(set(effs)) == len(effs), (name, fl, effs)
        assert W3.splits_s1(B, C, H, W, K, R, R, R // 2, 0, n + 7) == n          # the clamp to the chunk count


def test_row_cases_reach_idle_workgroups_and_several_per_xcd():
    B, C, H, W, K, R = W3.ROW_SHAPES["1x1_three_k_tiles"]
    assert 12 in W3.row_forced_list("1x1_three_k_tiles") and W3.row_grid(C, K, R, 12) == (40, 36, 4, 5)
    B, C, H, W, K, R = W3.ROW_SHAPES["5x5_idle_workgroup"]
    assert W3.row_grid(C, K, R, 1) == (16, 15, 1, 2) and W3.row_grid(C, K, R, 2) == (32, 30, 2, 4)
    grids = [W3.row_grid(C, K, R, W3.splits_s1(B, C, H, W, K, R, R, R // 2, 0, f))
             for name, (B, C, H, W, K, R) in W3.ROW_SHAPES.items() for f in W3.row_forced_list(name)]
    assert any(idle > 0 and nper > 1 for _, _, idle, nper in grids) and any(idle == 0 for _, _, idle, _ in grids)
    # rows that never meet the image, one live wavefront, H = 1
    B, C, H, W, K, R = W3.ROW_SHAPES["5x5_rows_outside"]
    assert [r for r in range(R) if not any(0 <= y + r - R // 2 < H for y in range(H))] == [0, 4]
    assert C % W3.RT_C == 32 and K % W3.RT_K == 32                         # the second c tile and the third k tile are half dead
    B, C, H, W, K, R = W3.ROW_SHAPES["5x5_one_row"]
    assert H == 1 and C == 32 and K == 32


def test_per_tap_cases_reach_one_and_two_chunks_and_both_loop_parities():
    def lens(g, forced):
        B, C, H, W, K, R, S, pad = g
        OH, OW = W3.out_hw(H, W, R, S, 1, pad)
        n = W3.nchunks_of(B, OH, OW)
        return [e - b for b, e in W3.chunk_ranges(n, W3.splits_s1(B, C, H, W, K, R, S, pad, 1, forced))]
    assert lens(W3.TAP_SHAPES["one_partial_chunk"], 0) == [1] and 3 * 3 < W3.PX
    assert lens(W3.TAP_SHAPES["two_chunks"], 0) == [2]
    assert lens(W3.TAP_SHAPES["33_chunks_ragged"], 2) == [17, 16] and (2 * 9 * 29) % W3.PX != 0
    assert lens(W3.TAP_SHAPES["33_chunks_ragged"], 3) == [17, 16]           # clamped: at least 16 chunks per split
    assert lens(W3.TAP_SHAPES["pad0_16x16_output"], 2) == [16, 16]
    B, C, H, W, K, R, S, pad = W3.TAP_SHAPES["dead_wavefronts"]
    assert (W3.cdiv(K, W3.TK), W3.cdiv(C, W3.TC)) == (3, 2) and K % W3.TK <= 64 and C % W3.TC <= 64
    for name, (B, C, H, W, K, R) in W3.ROW_SHAPES.items():                  # under wg3_row = 1: 16 chunks at the most, never split
        assert W3.splits_s1(B, C, H, W, K, R, R, R // 2, 1, 5) == 1, name
    B, C, H, W, K, R, st, pad = W3.STRIDED_SHAPES["s4_unread_pixels"]
    OH, OW = W3.out_hw(H, W, R, R, st, pad)
    read = {oy * st + r - pad for oy in range(OH) for r in range(R)}
    assert any(y not in read for y in range(H)), "every fine row is read"
    B, C, H, W, K, R, st, pad = W3.STRIDED_SHAPES["s2_odd_fine_grid"]
    assert H % 2 and W % 2


@pytest.mark.parametrize("M", [9, 48, 522])
def test_systematic_residual_inputs_expose_a_lost_cross_product(M):
    """numpy emulation of one output row: dw[k][c] = sum_m dy[m][k] x[m][c] with every operand as its two fp16 numbers, sums in
    float64.  a0.b0 + a0.b1 + a1.b0 must be within 1e-6 of the full product sum, relative to each output; without either cross
    term EVERY output must move by at least 3e-4 of itself (the gate of the GPU tests is 1e-4)."""
    x, dy = W3.resid((M, 8), 5, W3.X_EXP), W3.resid((M, 6), 6, W3.DY_EXP)
    assert x.min() > 0 and dy.min() > 0
    full = dy.astype(np.float64).T @ x.astype(np.float64)
    b0, b1, eb = W3.planes_of(x)
    a0, a1, ea = W3.planes_of(dy)
    assert (b1 > 0).all() and (a1 > 0).all(), "every second plane is positive"
    ulp = 16.0                                                               # of an fp16 number in [2^14, 2^15)
    assert np.abs(b1 / ulp - 0.45).max() < 0.01 and np.abs(a1 / ulp - 0.45).max() < 0.01
    fac = 2.0 ** -(ea + eb)
    three = (a0.T @ b0 + a0.T @ b1 + a1.T @ b0) * fac
    assert (np.abs(three - full) / full).max() <= 1e-6
    for what, lost in (("a1.b0", (a0.T @ b0 + a0.T @ b1) * fac), ("a0.b1", (a0.T @ b0 + a1.T @ b0) * fac)):
        moved = np.abs(lost - full) / full
        assert moved.min() >= 3e-4, (what, moved.min())
    # the integer inputs: both planes exact, the second one zero
    v = W3.ints((M, 8), 7, -8.0)
    p0, p1, e = W3.planes_of(v)
    assert e == 11 and not p1.any() and np.array_equal(p0 * 2.0 ** -e, v.astype(np.float64)) and np.abs(v).max() == 8
    assert 64 * 522 < 2 ** 24                                              # every partial sum of the largest case is an exact fp32 integer
