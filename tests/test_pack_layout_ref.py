"""CPU suite for tests/pack_layout_ref.py: the references that tests/test_hip_pack_layout.py holds the pack, slab-sum, bias-gradient
and layout kernels to are pinned here (the index formulas of include/stem_hip.h, torch's conv2d in float64, a-priori rounding
bounds), and every precondition the bit-for-bit GPU gates rest on is checked on the reference alone, case by case."""
import numpy as np
import pytest
import torch

import pack_layout_ref as ref


def _arange_weight(shape):
    return np.arange(1, int(np.prod(shape)) + 1, dtype=np.float32).reshape(shape)


# ------------------------------------------------------------------------------------------------------------------ pack_ref
@pytest.mark.parametrize("RS", [(2, 3), (5, 5)])
def test_pack_ref_index_identities(RS):
    """every element of every role against the header's formula: Conv2d [K,C,R,S] -> [R*S][K][C] (forward) / [R*S][C][K] (input
    gradient), ConvTranspose2d [C,K,R,S] -> the same two, C4: [K][32 taps][4] zero padded; the weight is left as it was"""
    R, S = RS
    K, C = 4, 3
    conv, deconv = _arange_weight((K, C, R, S)), _arange_weight((C, K, R, S))
    packed = {role: ref.pack_ref(deconv if role in (ref.PACK_DECONV_FWD, ref.PACK_DECONV_DGRAD) else conv, role)
              for role in ref.PACK_ROLES + [ref.PACK_CONV_FWD_C4]}
    for role, (p, after) in packed.items():
        assert np.array_equal(after, deconv if role in (ref.PACK_DECONV_FWD, ref.PACK_DECONV_DGRAD) else conv)
    assert packed[ref.PACK_CONV_FWD][0].shape == (R * S, K, C) and packed[ref.PACK_DECONV_DGRAD][0].shape == (R * S, C, K)
    assert packed[ref.PACK_CONV_FWD_C4][0].shape == (K, 32, 4)
    for k in range(K):
        for c in range(C):
            for r in range(R):
                for s in range(S):
                    t = r * S + s
                    assert packed[ref.PACK_CONV_FWD][0][t, k, c] == conv[k, c, r, s]
                    assert packed[ref.PACK_CONV_DGRAD][0][t, c, k] == conv[k, c, r, s]
                    assert packed[ref.PACK_DECONV_FWD][0][t, k, c] == deconv[c, k, r, s]
                    assert packed[ref.PACK_DECONV_DGRAD][0][t, c, k] == deconv[c, k, r, s]
                    assert packed[ref.PACK_CONV_FWD_C4][0][k, t, c] == conv[k, c, r, s]
    c4 = packed[ref.PACK_CONV_FWD_C4][0]
    assert not c4[:, R * S:, :].any() and not c4[:, :, C:].any() and np.count_nonzero(c4) == conv.size


@pytest.mark.parametrize("RS", [(2, 3), (5, 5), (3, 3), (3, 2)])
def test_pack_ref_masks(RS):
    """mask bits as the header states them: a tap is masked if row > R/2, or row == R/2 and col >= S/2 (type A) / col > S/2 (type B,
    bit 2).  Mode 1 masks the packed copy only, mode 2 the weight too -- and nothing but the masked taps; mode 0 ignores bit 2."""
    R, S = RS
    w = _arange_weight((3, 2, R, S))
    for typeb in (0, ref.MASK_B):
        live = np.array([[r < R // 2 or (r == R // 2 and s < S // 2 + (1 if typeb else 0)) for s in range(S)] for r in range(R)])
        assert np.array_equal(ref.mask_taps(R, S, 1 | typeb), ~live)
        for mode in (1, 2):
            for role in (ref.PACK_CONV_FWD, ref.PACK_CONV_DGRAD):
                p, after = ref.pack_ref(w, role, mode | typeb)
                assert np.array_equal(p, ref.pack_ref(w * live, role)[0])
                assert np.array_equal(after, w * live if mode == 2 else w)
        assert np.array_equal(ref.pack_ref(w, ref.PACK_CONV_FWD, typeb)[0], ref.pack_ref(w, ref.PACK_CONV_FWD)[0])
    if RS == (5, 5):            # the counts of a 5x5 MaskedConv2d: 12 live taps for type A, 13 for type B
        assert (~ref.mask_taps(5, 5, 1)).sum() == 12 and (~ref.mask_taps(5, 5, 1 | ref.MASK_B)).sum() == 13


@pytest.mark.parametrize("RS", [(2, 3), (5, 5)])
@pytest.mark.parametrize("deconv", [False, True])
def test_unpack_exact_round_trips_pack_ref(RS, deconv):
    """a weight packed for the forward role is one slab [t][K][C] (Conv2d) / for the DECONV input-gradient role one slab [t][C][K]
    (ConvTranspose2d): unpack_exact and unpack_f32 of that slab give the weight back"""
    R, S = RS
    K, C = 5, 3
    w = _arange_weight((C, K, R, S) if deconv else (K, C, R, S))
    slab = ref.pack_ref(w, ref.PACK_DECONV_DGRAD if deconv else ref.PACK_CONV_FWD)[0]
    assert np.array_equal(ref.unpack_exact(slab[None], K, C, R, S, deconv), w)
    assert np.array_equal(ref.unpack_f32(slab[None], K, C, R, S, deconv), w)


@pytest.mark.parametrize("typeb", [0, ref.MASK_B], ids=["A", "B"])
def test_masked_conv_from_pack_ref_taps(typeb):
    """a convolution built tap by tap from pack_ref's masked [t][K][C] copy == torch's conv2d with w * mask, float64, where the mask
    is the one MaskedConv2d builds (ones; [h//2, w//2 + (B):] and [h//2 + 1:] zeroed)"""
    rng = np.random.default_rng(5)
    K, C, R, S, H, W = 3, 2, 5, 5, 7, 8
    w, x = rng.standard_normal((K, C, R, S)), rng.standard_normal((1, C, H, W))
    mask = np.ones((R, S))
    mask[R // 2, S // 2 + (1 if typeb else 0):] = 0
    mask[R // 2 + 1:] = 0
    want = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w * mask), padding=(R // 2, S // 2)).numpy()
    p, _ = ref.pack_ref(w, ref.PACK_CONV_FWD, 1 | typeb)
    xp = np.pad(x, ((0, 0), (0, 0), (R // 2, R // 2), (S // 2, S // 2)))
    got = np.zeros((1, K, H, W))
    for r in range(R):
        for s in range(S):
            got += np.einsum("kc,bchw->bkhw", p[r * S + s], xp[:, :, r:r + H, s:s + W])
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert not np.array_equal(ref.pack_ref(w, ref.PACK_CONV_FWD, 1)[0], ref.pack_ref(w, ref.PACK_CONV_FWD, 1 | ref.MASK_B)[0])


# ------------------------------------------------------------------------------------------------------------------ layouts
def test_layout_references():
    x = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    y = ref.nchw_to_nhwc(x)
    assert y.shape == (2, 4, 5, 3) and all(y[b, h, w, c] == x[b, c, h, w] for b in range(2) for c in range(3) for h in range(4) for w in range(5))
    assert np.array_equal(ref.nhwc_to_nchw(y), x)
    got = ref.nhwc_to_nchw(ref.CLAMP_VALUES.reshape(1, 1, -1, 1), clamp01=True).reshape(-1)
    assert np.array_equal(got, np.array([0, 0, 0, 1e-30, 0, 0.5, 1 - 2.0 ** -24, 1, 1, 1, 1, 0, 1, 0], np.float32))


def test_nhwc4_record_layout():
    """word 0 = int slot count, word 1 = 1.0, words 2..15 zero, slot j = max |x| over the pixels [1024 j, 1024 (j + 1)) of the
    flattened B*H*W -- image boundaries inside a slot (3 x 700 pixels)"""
    B, H, W = 3, 20, 35
    x = np.random.default_rng(1).uniform(-1, 1, (B, 3, H, W)).astype(np.float32)
    x[1, 2, 16, 0] = -7.5            # flattened pixel 700 + 560 = 1260: slot 1
    y, q = ref.nhwc4_with_record(x)
    assert y.shape == (B, H, W, 4) and not y[..., 3].any() and np.array_equal(y[..., :3], x.transpose(0, 2, 3, 1))
    assert q.size == 16 + 3 and q[:1].view(np.int32)[0] == 3 and q[1] == 1.0 and not q[2:16].any()
    flat = np.abs(x.transpose(0, 2, 3, 1).reshape(-1, 3)).max(1)
    assert [q[16], q[17], q[18]] == [flat[:1024].max(), 7.5, flat[2048:].max()]
    assert ref.amax_record_max(q) == (3, 7.5)
    assert ref.amax_slots(1, 4, 5) == 1 and ref.amax_slots(2049, 32, 2000) == 9 and ref.amax_slots(70000, 100, 3) == 3
    assert ref.amax_slots(70000, 100, 2000) == 855


# ------------------------------------------------------------------------------------------------------------------ sums: bounds
def _slab_id(c):
    return "A%d_Bd%d_T%d_s%d_%s" % (c[0], c[1], c[2], c[3], "deconv" if c[4] else "conv")


@pytest.mark.parametrize("case", ref.UNPACK_CASES, ids=_slab_id)
def test_unpack_f32_within_the_a_priori_bound(case):
    """|unpack_f32 - unpack_exact| <= gamma_n * sum |x| element-wise, gamma_n = n u / (1 - n u), u = 2^-24, n = splits (+ 1 with
    ACCUMULATE): derived (Higham 4.2: any order of n terms is within gamma_(n-1)), not measured"""
    K, C, R, S = ref.unpack_kcrs(case)
    x = ref.unpack_slabs(case, "cancelling")
    exact = ref.unpack_exact(x, K, C, R, S, case[4])
    mag = ref.unpack_exact(np.abs(x), K, C, R, S, case[4])
    got = ref.unpack_f32(x, K, C, R, S, case[4])
    assert got.dtype == np.float32 and got.shape == exact.shape
    assert (np.abs(got - exact) <= ref.gamma(case[3]) * mag).all()
    old = ref.cancelling(exact.shape, 77)
    acc = ref.unpack_f32(x, K, C, R, S, case[4], old=old)
    assert acc.dtype == np.float32 and np.array_equal(acc, old + got)
    assert (np.abs(acc - (exact + old)) <= ref.gamma(case[3] + 1) * (mag + np.abs(old))).all()


def _bf_id(c):
    return "parts%d_K%d" % c


@pytest.mark.parametrize("case", ref.BIAS_FINAL_CASES, ids=_bf_id)
def test_colsum_final_f32_within_the_a_priori_bound(case):
    """the same bound for the second stage of the bias gradient, n = parts (+ 1 with accumulate)"""
    part = ref.bias_final_parts(case, "cancelling")
    exact, mag = part.astype(np.float64).sum(0), np.abs(part).astype(np.float64).sum(0)
    got = ref.colsum_final_f32(part)
    assert got.dtype == np.float32 and (np.abs(got - exact) <= ref.gamma(case[0]) * mag).all()
    old = ref.cancelling((case[1],), 78)
    acc = ref.colsum_final_f32(part, accumulate_into=old)
    assert np.array_equal(acc, old + got) and (np.abs(acc - (exact + old)) <= ref.gamma(case[0] + 1) * (mag + np.abs(old))).all()


def test_colsum_final_order():
    """the order itself, on an input where it shows: parts 0, 16, 32 share row group 0 and are added first.  (2^24 + 1) + -2^24 in
    that group gives 0 (the 1 is lost), the sequential order would keep a different value."""
    part = np.zeros((33, 1), np.float32)
    part[0], part[16], part[1] = 2.0 ** 24, 1.0, -2.0 ** 24
    assert ref.colsum_final_f32(part)[0] == 0.0                   # (2^24 + 1 -> 2^24) + (-2^24)
    part[16], part[2] = 0.0, 1.0
    assert ref.colsum_final_f32(part)[0] == 1.0                   # (2^24 - 2^24) + 1
    slabs = np.array([2.0 ** 24, -2.0 ** 24, 1.0], np.float32).reshape(3, 1, 1, 1)
    assert ref.unpack_f32(slabs, 1, 1, 1, 1)[0, 0, 0, 0] == 0.0   # (2^24 + 1 -> 2^24) + (-2^24): even slabs first
    assert ref.unpack_sequential_f32(slabs, 1, 1, 1, 1)[0, 0, 0, 0] == 1.0


# ------------------------------------------------------------------------------------------------------------------ preconditions of the GPU gates
def test_dyadic_grid():
    x = ref.dyadic((4096,), 3)
    assert x.dtype == np.float32 and np.array_equal(x * 8, np.rint(x * 8)) and x.min() == -8.0 and x.max() == 8.0
    assert ref.dyadic_is_exact(2 ** 17) and not ref.dyadic_is_exact(2 ** 18)
    # the claim behind dyadic_is_exact: float32 sums of such values equal the integer sum in any order
    y = ref.dyadic((2 ** 17,), 4)
    exact = float(y.astype(np.float64).sum())
    assert float(np.cumsum(y, dtype=np.float32)[-1]) == exact and float(np.cumsum(y[::-1], dtype=np.float32)[-1]) == exact
    assert float(y.sum(dtype=np.float32)) == exact                # numpy's pairwise order


def test_cancelling_spread():
    x = ref.cancelling((8, 4096), 5)
    lg = np.log10(np.abs(x))
    assert x.dtype == np.float32 and lg.min() < -1.9 and lg.max() > 1.9 and 0.4 < (x > 0).mean() < 0.6
    assert (lg.max(0) - lg.min(0)).mean() > 2.5                   # the spread is along the summed axis too


@pytest.mark.parametrize("case", ref.UNPACK_CASES, ids=_slab_id)
def test_unpack_case_preconditions(case):
    """(a) `dyadic` slabs sum exactly in fp32: max partial |sum| * 8 < 2^24 from the shape (splits + 1 terms with ACCUMULATE), and
    unpack_f32 == unpack_exact on them.  (b) `cancelling` slabs are order sensitive: the documented order and the plain
    sequential float32 sum differ in at least 5 % of the elements -- for splits >= 3; with one or two slabs there is only one
    order and the two are identical, which is asserted instead (those cases still run, against unpack_f32)."""
    A, Bd, T, splits, deconv = case
    K, C, R, S = ref.unpack_kcrs(case)
    assert ref.dyadic_is_exact(splits + 1)
    d = ref.unpack_slabs(case, "dyadic")
    assert np.array_equal(ref.unpack_f32(d, K, C, R, S, deconv), ref.unpack_exact(d, K, C, R, S, deconv))
    assert np.array_equal(ref.unpack_sequential_f32(d, K, C, R, S, deconv), ref.unpack_exact(d, K, C, R, S, deconv))
    x = ref.unpack_slabs(case, "cancelling")
    differ = float((ref.unpack_f32(x, K, C, R, S, deconv) != ref.unpack_sequential_f32(x, K, C, R, S, deconv)).mean())
    if ref.order_sensitive_slabs(splits):
        assert differ >= 0.05, differ
    else:
        assert differ == 0.0
    if (A, Bd) in ref.UNPACK_AUTO_MB:
        assert ref.unpack_auto_mb(A, Bd) == ref.UNPACK_AUTO_MB[(A, Bd)]
    else:
        assert ref.unpack_auto_mb(A, Bd) == 64


def test_unpack_case_list_covers_the_issue():
    """the geometries, tap counts, split counts and both layouts the slab-sum gates are meant to enter"""
    cs = ref.UNPACK_CASES
    assert {c[1] for c in cs} >= {3, 32, 37, 64, 100, 385} and {c[2] for c in cs} == {1, 4, 6, 9, 25}
    assert {c[3] for c in cs} == {1, 2, 3, 4, 5, 7, 8} and {c[4] for c in cs} == {False, True}
    assert sorted(ref.unpack_auto_mb(c[0], c[1]) for c in cs if c[0] == 512) == [96, 128, 160, 192]
    # float4 route (a full range of an aligned row) and scalar route (a partial range) inside one tensor
    assert any(c[1] % 4 == 0 and c[1] > 64 and c[1] % 64 for c in cs)
    assert len(ref.UNPACK_TABLE_CASES) == 33 and len(ref.PACK_MULTI_CASES) == 33 and len(ref.BIAS_FINAL_MULTI) == 25
    assert all(c in cs for c in ref.UNPACK_MISALIGNED_CASES)


@pytest.mark.parametrize("case", ref.BIAS_FINAL_CASES, ids=_bf_id)
def test_bias_final_case_preconditions(case):
    """the same two preconditions for the second stage: `dyadic` parts sum exactly (parts + 1 terms); `cancelling` parts are order
    sensitive in at least 5 % of the K elements for parts > 16 -- up to 16 parts every row group holds at most one part and the
    documented order IS the sequential one, asserted instead"""
    parts, K = case
    assert ref.dyadic_is_exact(parts + 1)
    d = ref.bias_final_parts(case, "dyadic")
    assert np.array_equal(ref.colsum_final_f32(d), d.astype(np.float64).sum(0))
    x = ref.bias_final_parts(case, "cancelling")
    differ = float((ref.colsum_final_f32(x) != ref.colsum_sequential_f32(x)).mean())
    if ref.order_sensitive_parts(parts):
        assert differ >= 0.05, differ
    else:
        assert differ == 0.0


def test_bias_grad_case_preconditions():
    """`dyadic` dy: npix + 1 terms per column are exact; the case list covers every npix, K and pitch kind, a float4-eligible and a
    scalar pitch per K % 4 == 0, and more than 16 parts at 5000 x 64"""
    cs = ref.BIAS_GRAD_CASES
    assert all(ref.dyadic_is_exact(npix + 1) for npix, _, _ in cs)
    assert {c[0] for c in cs} == set(ref.BIAS_NPIX) and {c[1] for c in cs} == set(ref.BIAS_K)
    assert all({kind for _, k, kind in cs if k == K} == set(ref.BIAS_PITCHES) for K in ref.BIAS_K)
    assert ref.bias_parts(5000, 64) == 40 and ref.bias_parts(1, 1) == 1 and ref.bias_parts(1000, 385) == 8
    for K in ref.BIAS_K:
        ld, c0 = ref.bias_pitch(K, "pad4")
        assert ld > K and ld % 4 == 0 and c0 == 0
        ld, c0 = ref.bias_pitch(K, "odd")
        assert ld > K and ld % 4 != 0 and c0 == 0
        ld, c0 = ref.bias_pitch(K, "slice1")
        assert ld >= K + 1 and ld % 4 == 0 and c0 == 1
    assert ref.BIAS_GRAD_CANCELLING in cs
