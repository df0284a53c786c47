"""CPU: the host side of the 192-column kernel's, the four-phase transposed form's and the first-layer kernel's tests -- the
get-only read-backs of the plans that ran ("fx3_col_ran_tile" | "fx3_col_ran_depth" | "fx3_col_ran_mfma"; "tconv_ran_tile" |
"tconv_ran_cps" | "tconv_ran_split0" .. "tconv_ran_split3"), the restated host arithmetic of tests/fx3_col_cases.py against the
numbers the issue of these kernels fixes (six instantiations, tap counts 9/6/6/4 and 4/2/2/1, cps and per-phase split counts, the
workspace need against stem_tconv2d_f16x3_workspace_bytes), and that case table itself: that it reaches every edge the GPU files
claim to run (chunk counts 1 .. 7, the XCD remap's remainder branch, a plan with exactly one split phase, ...).  Also the
statement the systematic-residual inputs rest on: dropping either cross product moves every output by more than the gate."""
import numpy as np
import pytest

import conv_ref as ref
import fx3_col_cases as K
from wg3_cases import planes_of

COL_RAN = (b"fx3_col_ran_tile", b"fx3_col_ran_depth", b"fx3_col_ran_mfma")
TCONV_RAN = (b"tconv_ran_tile", b"tconv_ran_cps", b"tconv_ran_split0", b"tconv_ran_split1", b"tconv_ran_split2", b"tconv_ran_split3")


@pytest.fixture(scope="module")
def lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


def test_read_backs_are_get_only(lib):
    import torch
    for name in COL_RAN + TCONV_RAN:
        before = lib.stem_tuning_get(name)
        assert before >= 0 and (before == 0 or torch.cuda.is_available()), name          # 0 until the family's first launch in this process
        assert lib.stem_tuning_set(name, before + 1) != 0 and name in lib.stem_last_error() and b"get-only" in lib.stem_last_error()
        assert lib.stem_tuning_set(name, 0) != 0 and lib.stem_tuning_get(name) == before
    assert lib.stem_tuning_get(b"tconv_ran_split4") == -1 and lib.stem_tuning_get(b"fx3_col_ran_form") == -1


def test_selectors_of_the_three_families_are_settable(lib):
    for name, good, bad in ((b"fx3_tile", (64, 128), 96), (b"fx3_depth", (2, 3), 4), (b"fx3_mfma", (16, 32), 8), (b"fx3_gen_tile", (64, 128), 32)):
        old = lib.stem_tuning_get(name)
        try:
            for v in good:
                assert lib.stem_tuning_set(name, v) == 0 and lib.stem_tuning_get(name) == v
            assert lib.stem_tuning_set(name, bad) != 0 and lib.stem_tuning_get(name) == good[-1]
        finally:
            lib.stem_tuning_set(name, old)
    old = lib.stem_tuning_get(b"tconv_cps")
    assert lib.stem_tuning_set(b"tconv_cps", 5) == 0 and lib.stem_tuning_get(b"tconv_cps") == 5 and lib.stem_tuning_set(b"tconv_cps", old) == 0


# ---- 192-column kernel ---------------------------------------------------------------------------------------------------------
def test_six_instantiations_and_the_ignored_selector():
    assert len(K.COL_FORMS) == 6
    assert {v[1] for v in K.COL_FORMS.values()} == {(bm, d, ms) for bm in (64, 128) for d, ms in ((2, 32), (3, 32), (3, 16))}
    for sel, want in K.COL_FORMS.values():
        assert K.col_instantiation(sel["fx3_tile"], sel["fx3_depth"], sel["fx3_mfma"]) == want
    for bm in (64, 128):
        assert K.col_instantiation(bm, 2, 16) == (bm, 2, 32)            # fx3_mfma = 16 with the two-stage loop runs 32
        assert len({K.col_instantiation(bm, d, ms) for d in (2, 3) for ms in (16, 32)}) == 3


def test_col_table_reaches_every_edge():
    S = K.COL_SHAPES
    chunk_counts = {K.col_chunks(C, R, Sx) for (B, C, H, W, N, R, Sx, st, pad) in S.values()}
    assert set(range(1, 8)) <= chunk_counts and 150 in chunk_counts
    assert {C for (B, C, *_) in [S[n] for n in S if K.col_chunks(S[n][1], S[n][5], S[n][6]) <= 7]} == {32, 64, 128}      # C = 96 as 1x1 is n = 3: reached by 1x3
    assert {N for (_, _, _, _, N, *_) in S.values()} >= {192, 100, 96, 64, 33}
    assert any(R != Sx for (*_, R, Sx, st, pad) in S.values()) and {Sx for (*_, R, Sx, st, pad) in S.values() if R == 1} >= {1, 3, 5, 7}
    assert {st for (*_, st, pad) in S.values()} >= {1, 2, 3}
    assert any(pad == 0 and (R > 1 or Sx > 1) for (*_, R, Sx, st, pad) in S.values()) and any(pad > max(R, Sx) // 2 for (*_, R, Sx, st, pad) in S.values())
    Ms = {n: np.prod([v[0], *K.out_hw(v[2], v[3], v[5], v[6], v[7], v[8])]) for n, v in S.items()}
    assert any(m < 64 for m in Ms.values())
    assert any(m % 64 and m % 128 and m > 128 for m in Ms.values())                       # an M tail on both tiles
    for n, v in S.items():                                                                # tiles that straddle rows and images
        OH, OW = K.out_hw(v[2], v[3], v[5], v[6], v[7], v[8])
        if n == "n3_1x3_pad0":
            assert 64 % OW and (OH * OW) % 64 and v[0] * OH * OW > OH * OW > 64
    for bm in (64, 128):                                                                  # >= 16 workgroups, not a multiple of 8
        nb = K.col_grid(*S["n1_xcd_remap"], bm)
        assert nb >= 16 and nb % 8, nb
        assert sorted(K.xcd_tile(bx, nb) for bx in range(nb)) == list(range(nb))          # the remap is a permutation
        assert any(K.xcd_tile(bx, nb) != bx for bx in range(nb))
    for v in S.values():
        B, C, H, W, N, R, Sx, st, pad = v
        assert C % 32 == 0 and N <= K.BN and R * Sx <= 25 and C * R * Sx * 64 < 2 ** 24   # integer inputs in [-8, 8] sum exactly in fp32
    assert set(K.COL_RESID) | set(K.COL_GDN) | set(K.COL_ACT) <= set(S)


@pytest.mark.parametrize("name", K.COL_RESID)
def test_dropping_a_cross_product_moves_every_output_by_more_than_the_gate(name):
    """with the systematic-residual operands x = x0 + x1, w = w0 + w1 (the two fp16 numbers of the planes): every output of
    conv(x1, w0) and of conv(x0, w1) exceeds 1e-4 of its channel's maximum -- a kernel that loses either product fails the gate"""
    B, C, H, W, N, R, Sx, st, pad = K.COL_SHAPES[name]
    x, w = K.col_resid_operands(name)
    x0, x1, ex = planes_of(x)
    w0, w1, ew = planes_of(w)
    assert np.array_equal((x0 + x1) * 2.0 ** -ex, x.astype(np.float64)) and np.array_equal((w0 + w1) * 2.0 ** -ew, w.astype(np.float64))
    full = ref.conv2d_fwd(x, w, None, st, pad)
    gate = 1e-4 * np.abs(full).max(axis=(0, 2, 3))[None, :, None, None]
    assert full.min() > 0
    for a, b in ((x1, w0), (x0, w1)):
        cross = ref.conv2d_fwd(a, b, None, st, pad) * 2.0 ** -(ex + ew)
        assert (np.abs(cross) > gate).all(), (name, float((np.abs(cross) / gate).min()))
    assert np.abs(ref.conv2d_fwd(x1, w1, None, st, pad) * 2.0 ** -(ex + ew)).max() < 1e-6 * np.abs(full).min()      # the dropped a1.b1 is nothing


# ---- four-phase transposed form ------------------------------------------------------------------------------------------------
def test_phase_tap_counts():
    assert K.tconv_taps(5) == [9, 6, 6, 4] and sorted(K.tconv_taps(3), reverse=True) == [4, 2, 2, 1] and K.tconv_taps(3) == [1, 2, 2, 4]
    for R in (3, 5):
        assert sum(K.tconv_taps(R)) == R * R
        for par in (0, 1):                                   # the taps of a parity: r = rmax, rmax - 2, ... reading coarse offsets d0, d0 + 1, ...
            cnt, d0, rmax = K.tconv_axis(R, R // 2, par)
            assert [(par + R // 2 - r) // 2 for r in range(rmax, -1, -2)] == list(range(d0, d0 + cnt))
            assert all((par + R // 2 - r) % 2 == 0 for r in range(rmax, -1, -2))


def test_cps_and_per_phase_splits():
    assert sorted(K.tconv_plan(32, 3, split=2)[1], reverse=True) == [2, 1, 1, 1]          # one phase splits, three do not
    assert K.tconv_plan(32, 3, split=2) == (2, [1, 1, 1, 2])
    assert K.tconv_plan(96, 5, split=3) == (9, [3, 2, 2, 2])                              # phases with different split counts under one z extent
    assert K.tconv_plan(96, 5, split=27) == (1, [27, 18, 18, 12]) == K.tconv_plan(96, 5, split=34)          # one chunk per workgroup; the clamp
    assert K.tconv_plan(64, 5, cps=5) == (5, [4, 3, 3, 2]) and K.tconv_plan(64, 5, split=2, cps=5) == (9, [2, 2, 2, 1])
    assert K.tconv_plan(64, 5, split=3, room=False) == (K.UNSPLIT_CPS, [1, 1, 1, 1]) and K.tconv_plan(64, 5, split=1, room=False) == (18, [1, 1, 1, 1])
    for C in (32, 64, 96):
        for R in (3, 5):
            nch, maxc = K.tconv_nch(C, R), max(K.tconv_nch(C, R))
            for s in range(1, maxc + 9):
                cps, ns = K.tconv_plan(C, R, split=s)
                assert cps == K.cdiv(maxc, min(s, maxc)) and ns == [K.cdiv(n, min(cps, n)) for n in nch]
                assert all((k - 1) * min(cps, n) < n for k, n in zip(ns, nch))            # no workgroup without a chunk


def test_workspace_need_against_the_library(lib):
    for name, (B, C, H, W, N, R, oh, ow) in K.TCONV_SHAPES.items():
        room = int(lib.stem_tconv2d_f16x3_workspace_bytes(B, H, W, C, N, R))
        assert room == K.tconv_room_bytes(B, H, W, N), name
        for s in K.tconv_split_list(C, R):
            ns = K.tconv_plan(C, R, split=s)[1]
            need = K.tconv_need_bytes(B, H, W, N, ns)
            assert need == K.CNT_BYTES + 4 * sum(n * B * H * W * K.cdiv(N, 128) * 128 for n in ns if n > 1)
            assert max(ns) > 16 or need <= room, (name, s)                                 # the room covers every plan of the planner (<= 16 slabs per phase)
            assert 4 * K.tconv_slots(B, H, W, N, 64) <= K.CNT_BYTES                        # one counter per workgroup of a z layer
    assert lib.stem_tconv2d_f16x3_workspace_bytes(2, 4, 4, 48, 96, 5) == 0 and lib.stem_tconv2d_f16x3_workspace_bytes(2, 4, 4, 64, 96, 4) == 0


def test_tconv_table_reaches_every_edge():
    S = K.TCONV_SHAPES
    Ms = [B * H * W for (B, C, H, W, *_) in S.values()]
    assert any(m < 64 for m in Ms) and all(m % 64 for m in Ms) and any(m > 128 and m % 128 for m in Ms)
    assert {v[1] for v in S.values()} == {32, 64, 96} and {v[4] for v in S.values()} == {96, 132, 160} and {v[5] for v in S.values()} == {3, 5}
    assert {(v[6], v[7]) for v in S.values()} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    vectors = {}
    for name, (B, C, H, W, N, R, oh, ow) in S.items():
        splits = K.tconv_split_list(C, R)
        maxc = max(K.tconv_nch(C, R))
        vs = [tuple(K.tconv_plan(C, R, split=s)[1]) for s in splits]
        assert len(set(vs)) == len(vs) and vs[0] == (1, 1, 1, 1) and vs[-1] == tuple(K.tconv_nch(C, R)), name
        assert tuple(K.tconv_plan(C, R, split=maxc + 7)[1]) == vs[-1]                      # a clamp at s > maxc
        vectors[name] = vs
    flat = [v for vs in vectors.values() for v in vs]
    assert (1, 1, 1, 2) in vectors["c32_r3_n96"]                                           # exactly one split phase (its slabs start at offset 0)
    assert any(len(set(v)) > 1 and min(v) > 1 for v in flat)                               # different split counts under one z extent
    assert any(min(v) == 1 < max(v) and sum(k > 1 for k in v) >= 2 for v in flat)          # an unsplit phase between split ones: the later one's wsofs counts
    assert any((oh or ow) and any(max(v) > 1 for v in vectors[n]) for n, (*_, oh, ow) in S.items())      # an odd fine grid together with a split
    for name, (B, C, H, W, N, R, oh, ow) in S.items():                                     # ragged ptiles on both tiles
        assert K.cdiv(B * H * W, 64) * 64 != B * H * W and K.cdiv(B * H * W, 128) * 128 != B * H * W


@pytest.mark.parametrize("name", list(K.TCONV_SHAPES))
def test_dropping_a_cross_product_moves_every_channel_of_the_transposed_face(name):
    """the phases of a transposed face have 1 .. 9 taps, so not EVERY output carries more than the gate in a cross product; every
    output of the phase with the most taps that has all of them inside the grid does (4e-4 of the channel's maximum), in every channel"""
    B, C, H, W, N, R, oh, ow = K.TCONV_SHAPES[name]
    x, w = K.tconv_resid_operands(name)
    x0, x1, ex = planes_of(x)
    w0, w1, ew = planes_of(w)
    shape = (B, N, 2 * H - oh, 2 * W - ow)
    full = ref.conv2d_dx(x, w, shape, 2, R // 2)
    cmax = np.abs(full).max(axis=(0, 2, 3))[None, :, None, None]
    assert full.min() > 0
    for a, b in ((x1, w0), (x0, w1)):
        cross = np.abs(ref.conv2d_dx(a, b, shape, 2, R // 2)) * 2.0 ** -(ex + ew)
        assert ((cross > 3e-4 * cmax).sum(axis=(0, 2, 3)) >= B).all(), name
        assert (cross[full > 0.9 * cmax] > 3e-4 * np.broadcast_to(cmax, full.shape)[full > 0.9 * cmax]).all(), name


@pytest.mark.parametrize("name", list(K.C4_SHAPES))
def test_dropping_a_cross_product_of_the_first_layer_moves_every_output(name):
    """through the GDN: with beta' >> gamma' v^2 the output follows v, so losing x1.w0 or x0.w1 of the convolution moves every
    output by more than 1e-4 of its channel's maximum -- except in channel 1, whose stored beta lies below its bound (beta' = 1e-6:
    there gamma' v^2 dominates and the output does not depend on the scale of v)"""
    B, H, W, N, R, S, st, pad = K.C4_SHAPES[name]
    x, w = K.c4_resid_operands(name)
    beta = np.random.default_rng(0).uniform(0.5, 1.5, N)
    beta[1] = 1e-4
    gamma = np.random.default_rng(1).uniform(0.0, 0.2, (N, N))
    x0, x1, ex = planes_of(x)
    w0, w1, ew = planes_of(w)
    v = ref.conv2d_fwd(x, w, None, st, pad)
    full = ref.gdn_fwd(v, beta, gamma)
    gate = 1e-4 * np.abs(full).max(axis=(0, 2, 3))[None, :, None, None]
    keep = np.arange(N) != 1
    for a, b in ((x1, w0), (x0, w1)):
        moved = np.abs(ref.gdn_fwd(v - ref.conv2d_fwd(a, b, None, st, pad) * 2.0 ** -(ex + ew), beta, gamma) - full)
        assert (moved[:, keep] > gate[:, keep]).all(), (name, float((moved / gate)[:, keep].min()))


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def test_pixel_steps_and_the_derived_amplitude_ratio():
    k = K.pixel_steps(200)
    assert k.max() == 16 and k.min() == 0 and np.array_equal(k[:64], k[64:128]) and set(k[:64]) == set(range(17))
    assert np.array_equal(K.square_split_error([0.0, 2.0 ** -20, 2.0 ** -3, 2.0 ** 13]), [2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -9])
    # 192-column kernel: the tile's maximum becomes 2^6 .. 2^7; below 2^-12.36 (worst case) / 2^-13.36 of it 1e-4 is no longer met
    assert abs(np.log2(K.amplitude_ratio_for(1e-4, 2.0 ** 6)) + 12.36) < 0.01 and abs(np.log2(K.amplitude_ratio_for(1e-4, 2.0 ** 7)) + 13.36) < 0.01
    # first-layer kernel: the BOUND of |conv output| becomes 2^7 .. 2^7.5 (its square 2^14 .. 2^15)
    assert abs(np.log2(K.amplitude_ratio_for(1e-4, 2.0 ** 7)) + 13.36) < 0.01 and abs(np.log2(K.amplitude_ratio_for(1e-4, 2.0 ** 7.5)) + 13.86) < 0.01


def test_first_layer_table_reaches_every_edge():
    S = K.C4_SHAPES
    assert {v[3] for v in S.values()} == {64, 128, 192} and {(v[4], v[5]) for v in S.values()} == {(1, 1), (3, 3), (5, 5), (3, 5)}
    assert {v[6] for v in S.values()} == {1, 2, 3} and any(v[7] == 0 and v[4] > 1 for v in S.values()) and any(v[7] == v[4] // 2 > 0 for v in S.values())
    Ms = {n: v[0] * np.prod(K.out_hw(v[1], v[2], v[4], v[5], v[6], v[7])) for n, v in S.items()}
    assert Ms["one_output_pixel"] == 1 and Ms["5x5_s2_n192"] > K.C4_WG and Ms["5x5_s2_n192"] % K.C4_WG
    assert K.out_hw(*[S["3x5_s2_long_rows"][i] for i in (1, 2, 4, 5, 6, 7)])[1] > K.C4_WG
