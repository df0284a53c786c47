"""GPU parity tests, op level, for the small HBM-bound kernels every training step ends in: the weight packs (stem_pack_weight,
stem_pack_weights_multi), the split-K slab sums (stem_unpack_wgrad, stem_unpack_wgrads_multi), the bias gradient (stem_bias_grad and
its second stage stem_bias_grad_final / _final_multi) and the layout kernels (stem_nchw_to_nhwc, stem_nhwc_to_nchw,
stem_copy_channels, stem_nchw3_to_nhwc4, stem_amax_nhwc).

These are permutations and fixed-order sums, so every comparison is np.array_equal against tests/pack_layout_ref.py (pinned on the
CPU by tests/test_pack_layout_ref.py, which also checks the preconditions: `dyadic` inputs sum exactly in fp32 in any order, so
the result must be the integer sum whatever the route; `cancelling` inputs round differently in different orders, so equality with
the documented order, between entry points and between run lengths is a statement about the order).  The one toleranced check
(stem_bias_grad on cancelling inputs) states its derived bound.  Every output buffer starts out as a NaN pattern; whatever the
kernel must not write -- pitch columns, the floats in front of and behind a view -- must still hold it afterwards."""
import numpy as np
import pytest
import torch

import pack_layout_ref as ref

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF            # a quiet NaN with a payload: no kernel produces it
GUARD = 64                   # sentinel floats behind (and in front of) a buffer; 64 floats keep the payload 16-byte aligned


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return functional


@pytest.fixture(scope="module")
def lib(F):
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


@pytest.fixture(scope="module")
def L():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def sent(n):
    return torch.full((int(n),), SENT, dtype=torch.int32, device="cuda").view(torch.float32)


def bits(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


def is_sent(t):
    return bool((bits(t) == SENT).all())


def guarded(a=None, n=None, front=GUARD):
    """-> (buffer, view): `front` sentinel floats, the payload (a copy of `a`, or n sentinel floats), GUARD sentinel floats"""
    n = int(a.size if a is not None else n)
    buf = sent(front + n + GUARD)
    view = buf[front:front + n]
    if a is not None:
        view.copy_(dev(a).reshape(-1))
    return buf, view


def guards_intact(buf, view):
    front = (view.data_ptr() - buf.data_ptr()) // 4
    return is_sent(buf[:front]) and is_sent(buf[front + view.numel():])


def host(view):
    return view.cpu().numpy()


# =========================================================================================================== 1. pack
def _weight(K, C, R, S, role, salt=0):
    """a weight without zeros (a masked tap shows), in the layout the role reads"""
    rng = np.random.default_rng(ref.case_seed(K, C, R, S, role, salt))
    shape = ref.pack_shape(K, C, R, S, role)
    return (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.25, 4.0, shape)).astype(np.float32)


def _pack_single(F, lib, w, K, C, R, S, role, masked):
    """stem_pack_weight on its own -> (packed, weight afterwards); nothing outside either buffer is written"""
    n = int(lib.stem_packed_weight_elems(K, C, R, S, role))
    wbuf, wv = guarded(w)
    obuf, ov = guarded(n=n)
    F._chk(lib.stem_pack_weight(wv.data_ptr(), ov.data_ptr(), K, C, R, S, role, masked, F._stream()))
    torch.cuda.synchronize()
    assert guards_intact(wbuf, wv) and guards_intact(obuf, ov)
    return host(ov), host(wv).reshape(w.shape)


def _pack_multi_one(F, L, w, K, C, R, S, role, masked):
    """the same through stem_pack_weights_multi with one descriptor"""
    wbuf, wv = guarded(w)
    obuf, ov = guarded(n=w.size)
    F.pack_weights_multi((L.PackDesc * 1)(L.PackDesc(wv.data_ptr(), ov.data_ptr(), K, C, R, S, role, masked)))
    torch.cuda.synchronize()
    assert guards_intact(wbuf, wv) and guards_intact(obuf, ov)
    return host(ov), host(wv).reshape(w.shape)


def _pack_id(c):
    return "K%d_C%d_%dx%d" % c


@pytest.mark.parametrize("role", ref.PACK_ROLES)
@pytest.mark.parametrize("shape", ref.PACK_SHAPES, ids=_pack_id)
def test_pack_weight_roles(F, lib, L, shape, role):
    """the four transposing roles: Conv2d [K,C,R,S] / ConvTranspose2d [C,K,R,S] -> [R*S][K][C] and [R*S][C][K]; square, 1x1 and
    rectangular filters, rows of 385 floats (more than one pass of the 256 threads), one to 385 workgroups"""
    K, C, R, S = shape
    w = _weight(K, C, R, S, role)
    want, _ = ref.pack_ref(w, role)
    got, after = _pack_single(F, lib, w, K, C, R, S, role, 0)
    assert np.array_equal(got, want.reshape(-1)) and np.array_equal(after, w)
    assert np.array_equal(host(F.pack_weight(dev(w), role)), want.reshape(-1))
    multi, after = _pack_multi_one(F, L, w, K, C, R, S, role, 0)
    assert np.array_equal(multi, got) and np.array_equal(after, w)


@pytest.mark.parametrize("shape", ref.PACK_C4_CASES, ids=_pack_id)
def test_pack_weight_c4(F, lib, shape):
    """first-layer role: [K][3 or 4][R*S] -> [K][32 taps][4], zero padded in both the tap and the channel direction"""
    K, C, R, S = shape
    w = _weight(K, C, R, S, ref.PACK_CONV_FWD_C4)
    want, _ = ref.pack_ref(w, ref.PACK_CONV_FWD_C4)
    got, after = _pack_single(F, lib, w, K, C, R, S, ref.PACK_CONV_FWD_C4, 0)
    assert got.size == K * 128 and np.array_equal(got, want.reshape(-1)) and np.array_equal(after, w)


@pytest.mark.parametrize("role", ref.PACK_ROLES)
@pytest.mark.parametrize("masked", ref.PACK_MASKS, ids=["A1", "A2", "B1", "B2"])
@pytest.mark.parametrize("shape", ref.PACK_MASKED_SHAPES, ids=_pack_id)
def test_pack_weight_masked(F, lib, L, shape, masked, role):
    """modes 1 and 2, types A and B, 5x5 / 3x3 / 2x3 / 3x2 filters, every role (DGRAD: one workgroup's in-place writes to the weight
    interleave with the other rows').  Mode 1 leaves the weight untouched; mode 2 zeroes its masked taps and changes nothing else."""
    K, C, R, S = shape
    w = _weight(K, C, R, S, role)
    want, want_after = ref.pack_ref(w, role, masked)
    got, after = _pack_single(F, lib, w, K, C, R, S, role, masked)
    assert np.array_equal(got, want.reshape(-1))
    assert np.array_equal(after, want_after)
    assert np.array_equal(after, w) == ((masked & 3) == 1)
    multi, multi_after = _pack_multi_one(F, L, w, K, C, R, S, role, masked)
    assert np.array_equal(multi, got) and np.array_equal(multi_after, after)
    assert (want == 0).sum() == K * C * int(ref.mask_taps(R, S, masked).sum()) > 0


def test_pack_weight_lds_limits(F, lib, L):
    """a per-row slab of 67200 B (> 64 KiB: the dynamic-LDS attribute branch) packs like any other, single and multi; one of
    170000 B (> 160 KiB) is an error from both entry points and nothing is launched"""
    K, C, R, S, role, masked = ref.PACK_LDS_BIG
    assert 64 * 1024 < C * R * S * 4 <= 160 * 1024
    w = _weight(K, C, R, S, role)
    want, want_after = ref.pack_ref(w, role, masked)
    got, after = _pack_single(F, lib, w, K, C, R, S, role, masked)
    assert np.array_equal(got, want.reshape(-1)) and np.array_equal(after, want_after)
    multi, multi_after = _pack_multi_one(F, L, w, K, C, R, S, role, masked)
    assert np.array_equal(multi, got) and np.array_equal(multi_after, after)
    K, C, R, S, role, masked = ref.PACK_LDS_OVER
    assert C * R * S * 4 > 160 * 1024
    w = _weight(K, C, R, S, role)
    wbuf, wv = guarded(w)
    obuf, ov = guarded(n=w.size)
    with pytest.raises(RuntimeError, match="exceeds LDS"):
        F._chk(lib.stem_pack_weight(wv.data_ptr(), ov.data_ptr(), K, C, R, S, role, masked, F._stream()))
    with pytest.raises(RuntimeError, match="exceeds LDS"):
        F.pack_weights_multi((L.PackDesc * 1)(L.PackDesc(wv.data_ptr(), ov.data_ptr(), K, C, R, S, role, masked)))
    torch.cuda.synchronize()
    assert is_sent(obuf) and np.array_equal(host(wv), w.reshape(-1))


def test_pack_weights_multi_33(F, lib, L):
    """33 descriptors in one call: the table is split at 32 (two launches).  Roles, tap counts and masks mixed, the > 64 KiB slab
    among them (every workgroup of that launch then runs with the large LDS size).  Packed copies and weights afterwards equal the
    single-call results bit for bit, and the reference."""
    cases = ref.PACK_MULTI_CASES
    ws = [_weight(K, C, R, S, role, salt=i) for i, (K, C, R, S, role, masked) in enumerate(cases)]
    wbufs = [guarded(w) for w in ws]
    obufs = [guarded(n=w.size) for w in ws]
    descs = (L.PackDesc * len(cases))(*[L.PackDesc(wv.data_ptr(), ov.data_ptr(), *c) for c, (_, wv), (_, ov) in zip(cases, wbufs, obufs)])
    F.pack_weights_multi(descs)
    torch.cuda.synchronize()
    for i, (c, w, (wbuf, wv), (obuf, ov)) in enumerate(zip(cases, ws, wbufs, obufs)):
        K, C, R, S, role, masked = c
        want, want_after = ref.pack_ref(w, role, masked)
        single, single_after = _pack_single(F, lib, w, *c)
        assert guards_intact(wbuf, wv) and guards_intact(obuf, ov), (i, c)
        assert np.array_equal(host(ov), single) and np.array_equal(single, want.reshape(-1)), (i, c)
        assert np.array_equal(host(wv).reshape(w.shape), single_after) and np.array_equal(single_after, want_after), (i, c)


# =========================================================================================================== 2. slab sums
def _slab_id(c):
    return "A%d_Bd%d_T%d_s%d_%s" % (c[0], c[1], c[2], c[3], "deconv" if c[4] else "conv")


def _flags(case, accumulate=False):
    return (ref.UNPACK_DECONV if case[4] else 0) | (ref.UNPACK_ACCUMULATE if accumulate else 0)


def _unpack(F, lib, L, entry, dwp, dw, case, flags):
    K, C, R, S = ref.unpack_kcrs(case)
    if entry == "single":
        F._chk(lib.stem_unpack_wgrad(dwp.data_ptr(), dw.data_ptr(), K, C, R, S, case[3], flags, F._stream()))
    else:
        F.unpack_wgrads_multi((L.UnpackDesc * 1)(L.UnpackDesc(dwp.data_ptr(), dw.data_ptr(), K, C, R, S, case[3], flags)))


def _run_unpack(F, lib, L, entry, slabs, case, old=None, accumulate=False, front_dwp=GUARD, front_dw=GUARD):
    """one slab sum through `entry` ("single" / "multi") -> dw [A][Bd][R][S]; dw starts as the NaN pattern, or as `old`"""
    K, C, R, S = ref.unpack_kcrs(case)
    pbuf, pv = guarded(slabs, front=front_dwp)
    dbuf, dv = guarded(old, n=K * C * R * S, front=front_dw)
    _unpack(F, lib, L, entry, pv, dv, case, _flags(case, accumulate))
    torch.cuda.synchronize()
    assert guards_intact(dbuf, dv) and guards_intact(pbuf, pv) and np.array_equal(host(pv), slabs.reshape(-1))
    return host(dv).reshape((C, K, R, S) if case[4] else (K, C, R, S))


@pytest.mark.parametrize("case", ref.UNPACK_CASES, ids=_slab_id)
def test_unpack_dyadic_is_the_integer_sum(F, lib, L, case):
    """check (a), the semantics: on slabs whose sums are exact in fp32 in any order, both entry points give the exact sum in the
    reference layout (Conv2d [K,C,R,S] / ConvTranspose2d [C,K,R,S]) -- no slab dropped, none counted twice, at any run length"""
    K, C, R, S = ref.unpack_kcrs(case)
    slabs = ref.unpack_slabs(case, "dyadic")
    want = ref.unpack_exact(slabs, K, C, R, S, case[4])
    assert np.array_equal(_run_unpack(F, lib, L, "single", slabs, case), want)
    assert np.array_equal(_run_unpack(F, lib, L, "multi", slabs, case), want)
    for mb in (32, 192):
        with F.tuning(unpack_mb=mb):
            assert np.array_equal(_run_unpack(F, lib, L, "multi", slabs, case), want), mb
    assert lib.stem_tuning_get(b"unpack_mb") == 0


@pytest.mark.parametrize("case", ref.UNPACK_CASES, ids=_slab_id)
def test_unpack_cancelling_follows_the_documented_order(F, lib, L, case):
    """check (b), the order: on slabs whose rounded sum depends on the order, the single-tensor kernel, and the multi kernel at its
    automatic run length and at every forced one (float4 route where a full range of an aligned row allows it, scalar route
    elsewhere -- both inside one tensor for Bd = 100), all give unpack_f32: even slabs into one accumulator, odd slabs into the
    other, the result their sum.  The setting is restored on exit."""
    K, C, R, S = ref.unpack_kcrs(case)
    slabs = ref.unpack_slabs(case, "cancelling")
    want = ref.unpack_f32(slabs, K, C, R, S, case[4])
    assert np.array_equal(_run_unpack(F, lib, L, "single", slabs, case), want), "single"
    for mb in ref.UNPACK_MB_VALUES:
        with F.tuning(unpack_mb=mb):
            assert lib.stem_tuning_get(b"unpack_mb") == mb
            got = _run_unpack(F, lib, L, "multi", slabs, case)
        assert lib.stem_tuning_get(b"unpack_mb") == 0
        assert np.array_equal(got, want), f"multi unpack_mb={mb}: {(got != want).sum()} of {want.size} differ"


@pytest.mark.parametrize("case", ref.UNPACK_CASES, ids=_slab_id)
def test_unpack_accumulate(F, lib, L, case):
    """check (c): with STEM_UNPACK_ACCUMULATE a pre-filled gradient becomes old + sum (the sum rounded first, then one more
    rounding); without the flag the sum overwrites it"""
    K, C, R, S = ref.unpack_kcrs(case)
    slabs = ref.unpack_slabs(case, "cancelling")
    old = ref.cancelling((K * C * R * S,), ref.case_seed(*case[:4], 99))
    want = ref.unpack_f32(slabs, K, C, R, S, case[4])
    want_acc = ref.unpack_f32(slabs, K, C, R, S, case[4], old=old)
    assert (want_acc != want).mean() > 0.9
    for entry in ("single", "multi"):
        assert np.array_equal(_run_unpack(F, lib, L, entry, slabs, case, old=old, accumulate=True), want_acc), entry
        assert np.array_equal(_run_unpack(F, lib, L, entry, slabs, case, old=old), want), entry
    d = ref.unpack_slabs(case, "dyadic")
    dold = ref.dyadic((K * C * R * S,), 98)
    want = ref.unpack_exact(d, K, C, R, S, case[4]) + dold.reshape(want.shape)
    with F.tuning(unpack_mb=128):
        assert np.array_equal(_run_unpack(F, lib, L, "multi", d, case, old=dold, accumulate=True), want)


@pytest.mark.parametrize("which", ["dwp", "dw", "both"])
@pytest.mark.parametrize("case", ref.UNPACK_MISALIGNED_CASES, ids=_slab_id)
def test_unpack_misaligned_views(F, lib, L, case, which):
    """shapes that qualify for the float4 route, but the slabs and / or the gradient are views that start one float into a larger
    buffer (4 bytes off a 16-byte boundary): the scalar route must be taken, the sums are the same bits, and the floats in front
    of and behind the views are untouched"""
    K, C, R, S = ref.unpack_kcrs(case)
    assert case[1] % 4 == 0 and (case[0] * case[1] * case[2]) % 4 == 0
    slabs = ref.unpack_slabs(case, "cancelling")
    want = ref.unpack_f32(slabs, K, C, R, S, case[4])
    old = ref.cancelling((want.size,), 97)
    fp, fd = (GUARD + 1 if which in ("dwp", "both") else GUARD), (GUARD + 1 if which in ("dw", "both") else GUARD)
    for entry in ("single", "multi"):
        assert np.array_equal(_run_unpack(F, lib, L, entry, slabs, case, front_dwp=fp, front_dw=fd), want), entry
    with F.tuning(unpack_mb=128):
        assert np.array_equal(_run_unpack(F, lib, L, "multi", slabs, case, front_dwp=fp, front_dw=fd), want)
    got = _run_unpack(F, lib, L, "multi", slabs, case, old=old, accumulate=True, front_dwp=fp, front_dw=fd)
    assert np.array_equal(got, ref.unpack_f32(slabs, K, C, R, S, case[4], old=old))


def test_unpack_wgrads_multi_33(F, lib, L):
    """33 descriptors in one call (the table is split at 32): every small geometry, two of the 512-row ones, both layouts, with and
    without ACCUMULATE, aligned and misaligned gradients -- each result equals unpack_f32 and the single-tensor kernel's"""
    table = ref.UNPACK_TABLE_CASES
    items = []
    for i, (case, acc, misaligned) in enumerate(table):
        K, C, R, S = ref.unpack_kcrs(case)
        slabs = ref.unpack_slabs(case, "cancelling", salt=i)
        old = ref.cancelling((K * C * R * S,), 1000 + i) if acc else None
        pbuf, pv = guarded(slabs)
        dbuf, dv = guarded(old, n=K * C * R * S, front=GUARD + (1 if misaligned else 0))
        items.append((case, slabs, old, pbuf, pv, dbuf, dv, _flags(case, bool(acc))))
    descs = (L.UnpackDesc * len(items))(*[L.UnpackDesc(pv.data_ptr(), dv.data_ptr(), *ref.unpack_kcrs(case), case[3], flags)
                                         for case, _, _, _, pv, _, dv, flags in items])
    F.unpack_wgrads_multi(descs)
    torch.cuda.synchronize()
    for i, (case, slabs, old, pbuf, pv, dbuf, dv, flags) in enumerate(items):
        K, C, R, S = ref.unpack_kcrs(case)
        want = ref.unpack_f32(slabs, K, C, R, S, case[4], old=old)
        assert guards_intact(dbuf, dv) and guards_intact(pbuf, pv), (i, case)
        assert np.array_equal(host(dv).reshape(want.shape), want), (i, case)
        assert np.array_equal(_run_unpack(F, lib, L, "single", slabs, case, old=old, accumulate=old is not None), want), (i, case)


# =========================================================================================================== 3. bias gradient
def _bf_id(c):
    return "parts%d_K%d" % c


def _bias_final(F, lib, L, entry, part, old=None):
    parts, K = part.shape
    pbuf, pv = guarded(part)
    dbuf, dv = guarded(old, n=K)
    if entry == "single":
        F._chk(lib.stem_bias_grad_final(pv.data_ptr(), K, parts, dv.data_ptr(), int(old is not None), F._stream()))
    else:
        F.bias_grad_final_multi([L.BiasFinalDesc(pv.data_ptr(), dv.data_ptr(), K, parts, int(old is not None), 0)])
    torch.cuda.synchronize()
    assert guards_intact(dbuf, dv) and guards_intact(pbuf, pv)
    return host(dv)


@pytest.mark.parametrize("case", ref.BIAS_FINAL_CASES, ids=_bf_id)
def test_bias_grad_final(F, lib, L, case):
    """second stage on its own, both entry points: `dyadic` parts give the exact column sum (every part counted once, whatever the
    order), `cancelling` parts give colsum_final_f32 bit for bit (row group r sums parts r, r + 16, ... from 0, the 16 group sums are
    added in order); with accumulate the result is old + that"""
    d = ref.bias_final_parts(case, "dyadic")
    x = ref.bias_final_parts(case, "cancelling")
    old = ref.cancelling((case[1],), ref.case_seed(*case, 5))
    dold = ref.dyadic((case[1],), ref.case_seed(*case, 6))
    for entry in ("single", "multi"):
        assert np.array_equal(_bias_final(F, lib, L, entry, d), d.astype(np.float64).sum(0)), entry
        assert np.array_equal(_bias_final(F, lib, L, entry, d, old=dold), d.astype(np.float64).sum(0) + dold), entry
        assert np.array_equal(_bias_final(F, lib, L, entry, x), ref.colsum_final_f32(x)), entry
        assert np.array_equal(_bias_final(F, lib, L, entry, x, old=old), ref.colsum_final_f32(x, accumulate_into=old)), entry


def test_bias_grad_final_multi_25(F, lib, L):
    """25 descriptors through F.bias_grad_final_multi = two launches (24 + 1).  The widest tensor (K = 385: seven 64-column blocks)
    sits next to K = 1 and K = 63, whose workgroups beyond the first return early.  Multi equals single bit for bit, and the
    reference."""
    items = []
    for i, (parts, K, acc) in enumerate(ref.BIAS_FINAL_MULTI):
        x = ref.cancelling((parts, K), ref.case_seed(parts, K, acc, i))
        old = ref.cancelling((K,), 2000 + i) if acc else None
        items.append((x, old) + guarded(x) + guarded(old, n=K))
    F.bias_grad_final_multi([L.BiasFinalDesc(pv.data_ptr(), dv.data_ptr(), x.shape[1], x.shape[0], int(old is not None), 0)
                             for x, old, _, pv, _, dv in items])
    torch.cuda.synchronize()
    for i, (x, old, pbuf, pv, dbuf, dv) in enumerate(items):
        assert guards_intact(dbuf, dv) and guards_intact(pbuf, pv), i
        single = _bias_final(F, lib, L, "single", x, old=old)
        assert np.array_equal(host(dv), single) and np.array_equal(single, ref.colsum_final_f32(x, accumulate_into=old)), (i, x.shape)


def _dy(a, ld, c0):
    """[npix, K] numpy -> ([1,K,1,npix] device view with NHWC memory: channels c0 .. c0 + K of rows ld floats wide, the other
    columns hold 1e30), the buffer"""
    npix, K = a.shape
    buf = torch.full((npix, ld), 1e30, dtype=torch.float32, device="cuda")
    buf[:, c0:c0 + K] = dev(a)
    return buf.view(1, 1, npix, ld).permute(0, 3, 1, 2)[:, c0:c0 + K], buf


def _bg_id(c):
    return "npix%d_K%d_%s" % c


@pytest.mark.parametrize("case", ref.BIAS_GRAD_CASES, ids=_bg_id)
def test_bias_grad_dyadic_exact(F, lib, case):
    """stem_bias_grad from dy, both stages: pixel counts around the 128-row part and the 64-row unrolled loop with its 16-row
    tail, 40 parts at 5000 x 64 (more than the 16 row groups of the second stage); K around the float4 and the 64-column tile;
    pitches ld = K, ld > K (multiple of 4 and not) and a channel slice that starts at channel 1 (the float4 route needs K % 4 == 0,
    ld % 4 == 0 and a 16-byte aligned base).  Pitch columns hold 1e30: one of them read shows.  `dyadic` dy: the result is the
    integer column sum exactly, overwriting and accumulating."""
    npix, K, kind = case
    ld, c0 = ref.bias_pitch(K, kind)
    a = ref.dyadic((npix, K), ref.case_seed(npix, K, ld, c0))
    dy, buf = _dy(a, ld, c0)
    assert F.nhwc_ld(dy) == (ld if npix > 1 else K) and (dy.data_ptr() % 16 == 0) == (c0 == 0)
    assert int(lib.stem_bias_grad_scratch_elems(npix, K)) == ref.bias_parts(npix, K) * K
    want = a.astype(np.float64).sum(0)
    dbuf, db = guarded(n=K)
    F.bias_grad(dy, db)
    assert np.array_equal(host(db), want) and guards_intact(dbuf, db)
    old = ref.dyadic((K,), 7)
    dbuf, db = guarded(old)
    F.bias_grad(dy, db, accumulate=True)
    assert np.array_equal(host(db), want + old) and guards_intact(dbuf, db)
    keep = torch.ones(ld, dtype=torch.bool)
    keep[c0:c0 + K] = False
    assert bool((buf.cpu()[:, keep] == 1e30).all()) and np.array_equal(buf.cpu().numpy()[:, c0:c0 + K], a)


@pytest.mark.parametrize("kind", ref.BIAS_PITCHES)
def test_bias_grad_cancelling_within_the_summation_bound(F, kind):
    """the one toleranced check: `cancelling` dy against the float64 column sum within gamma_n * sum |dy|, gamma_n = n u / (1 - n u),
    u = 2^-24, n = npix (+ 1 with accumulate) -- the a-priori bound of ANY summation order of n terms (Higham 4.2), so it holds for
    both routes and any part count"""
    npix, K, _ = ref.BIAS_GRAD_CANCELLING
    ld, c0 = ref.bias_pitch(K, kind)
    a = ref.cancelling((npix, K), 4242)
    dy, _ = _dy(a, ld, c0)
    exact, mag = a.astype(np.float64).sum(0), np.abs(a).astype(np.float64).sum(0)
    db = sent(K)
    F.bias_grad(dy, db)
    err = np.abs(host(db).astype(np.float64) - exact)
    print(f"[bias_grad cancelling] {kind}: max err / (gamma_n sum|dy|) = {(err / (ref.gamma(npix) * mag)).max():.3e}")
    assert (err <= ref.gamma(npix) * mag).all()
    old = ref.cancelling((K,), 4243)
    db = dev(old)
    F.bias_grad(dy, db, accumulate=True)
    err = np.abs(host(db).astype(np.float64) - (exact + old))
    assert (err <= ref.gamma(npix + 1) * (mag + np.abs(old))).all()


# =========================================================================================================== 4. layouts
def _t_id(c):
    return "B%d_C%d_%dx%d" % c


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("shape", ref.TRANSPOSE_CASES, ids=_t_id)
def test_nchw_to_nhwc(F, lib, shape, pad):
    """[B][C][HW] -> [B][HW][ld] with C and HW off the 32 x 32 tile, a single element, and full tiles; destination pitch ld = C and
    ld = C + 3 (the library entry directly: F.to_nhwc always uses ld = C).  Exact; pitch columns and the floats behind the
    buffer are untouched."""
    B, C, H, W = shape
    x = np.random.default_rng(ref.case_seed(*shape)).standard_normal(shape).astype(np.float32)
    ld = C + pad
    ybuf, yv = guarded(n=B * H * W * ld)
    xd = dev(x)
    F._chk(lib.stem_nchw_to_nhwc(xd.data_ptr(), yv.data_ptr(), ld, B, C, H, W, F._stream()))
    torch.cuda.synchronize()
    y = yv.view(B * H * W, ld)
    assert np.array_equal(host(y[:, :C]), ref.nchw_to_nhwc(x).reshape(-1, C))
    assert guards_intact(ybuf, yv) and (pad == 0 or is_sent(y[:, C:]))
    if pad == 0:
        t = F.to_nhwc(xd)
        assert F.nhwc_ld(t) == C and np.array_equal(host(t.permute(0, 2, 3, 1)), ref.nchw_to_nhwc(x))


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("shape", ref.TRANSPOSE_CASES, ids=_t_id)
def test_nhwc_to_nchw(F, lib, shape, clamp):
    """[B][HW][ld] -> [B][C][HW] from a channel slice (channels 2 .. 2 + C of rows C + 5 wide, NaN pattern around it): exact, nothing
    behind the output written.  clamp01: min(max(v, 0), 1) on values straddling 0 and 1 -- -0.0, 0, 1, the neighbours of 1, huge
    values and infinities among them (the sign of a zero result is not compared)."""
    B, C, H, W = shape
    rng = np.random.default_rng(ref.case_seed(*shape, 1))
    x = rng.uniform(-0.5, 1.5, (B, H, W, C)).astype(np.float32)
    pick = rng.random(x.shape) < 0.5
    x[pick] = rng.choice(ref.CLAMP_VALUES, int(pick.sum()))
    ld = C + 5
    src = sent(B * H * W * ld).view(B, H, W, ld)
    src[..., 2:2 + C] = dev(x)
    view = src.permute(0, 3, 1, 2)[:, 2:2 + C]
    want = ref.nhwc_to_nchw(x, clamp)
    ybuf, yv = guarded(n=x.size)
    F._chk(lib.stem_nhwc_to_nchw(view.data_ptr(), ld, yv.data_ptr(), B, C, H, W, int(clamp), F._stream()))
    torch.cuda.synchronize()
    assert np.array_equal(host(yv).reshape(want.shape), want) and guards_intact(ybuf, yv)
    if B * H * W > 1:
        assert F.nhwc_ld(view) == ld
    got = host(F.to_nchw(view, clamp01=clamp))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not clamp or (got.min() >= 0.0 and got.max() <= 1.0)
    keep = torch.ones(ld, dtype=torch.bool)
    keep[2:2 + C] = False
    assert is_sent(src[..., keep])


def test_clamp01_known_values(F):
    vals = ref.CLAMP_VALUES
    x = sent(vals.size * 8).view(1, 1, vals.size, 8)
    x[..., 3:4] = dev(vals).view(1, 1, -1, 1)
    got = host(F.to_nchw(x.permute(0, 3, 1, 2)[:, 3:4], clamp01=True)).reshape(-1)
    assert np.array_equal(got, np.array([0, 0, 0, 1e-30, 0, 0.5, 1 - 2.0 ** -24, 1, 1, 1, 1, 0, 1, 0], np.float32))
    assert np.array_equal(host(F.to_nchw(x.permute(0, 3, 1, 2)[:, 3:4])).reshape(-1).view(np.uint32), vals.view(np.uint32))


@pytest.mark.parametrize("C", ref.COPY_CHANNELS_C)
def test_copy_channels_touches_only_its_slice(F, C):
    """source and destination are channel slices of wider buffers (pitches C + 7 and C + 5): the slice is copied bit for bit and
    every other float of the destination buffer keeps the NaN pattern"""
    B, H, W = 2, 7, 9                                    # 126 pixels: 126 * C is no multiple of the 256-thread workgroup
    x = np.random.default_rng(C).standard_normal((B, H, W, C)).astype(np.float32)
    sbuf = sent(B * H * W * (C + 7)).view(B, H, W, C + 7)
    sbuf[..., 3:3 + C] = dev(x)
    dbuf = sent(B * H * W * (C + 5) + GUARD)
    d4 = dbuf[:B * H * W * (C + 5)].view(B, H, W, C + 5)
    out = F.copy_channels(sbuf.permute(0, 3, 1, 2)[:, 3:3 + C], d4.permute(0, 3, 1, 2)[:, 2:2 + C])
    assert out.data_ptr() == d4.data_ptr() + 8
    assert np.array_equal(host(d4[..., 2:2 + C]), x)
    keep = torch.ones(C + 5, dtype=torch.bool)
    keep[2:2 + C] = False
    assert is_sent(d4[..., keep]) and is_sent(dbuf[B * H * W * (C + 5):])


@pytest.mark.parametrize("shape", ref.NHWC4_CASES, ids=lambda s: "B%d_%dx%d" % s)
def test_nchw3_to_nhwc4_and_its_record(F, lib, shape):
    """pixels exact with a zero fourth component; the scale record byte-equal to the reference's: int slot count, 1.0, fourteen
    zeroed words, and EVERY slot = max |x| of its 1024 flattened pixels (1, 255, 1024, 1025 pixels; 3 x 700: image boundaries inside
    a slot).  These slots are what the first-layer fp16 kernel scales by.  Nothing behind the image or the record is written."""
    B, H, W = shape
    npix = B * H * W
    rng = np.random.default_rng(ref.case_seed(*shape))
    x = (rng.standard_normal((B, 3, H, W)) * 10.0 ** rng.uniform(-3, 1, (B, 1, H, W))).astype(np.float32)
    x.reshape(-1)[rng.integers(0, x.size)] = -123.5                 # the maximum sits in one slot only
    want_y, want_q = ref.nhwc4_with_record(x)
    assert want_q.size == int(lib.stem_nhwc4_qrec_floats(B, H, W))
    xd = dev(x)
    ybuf, yv = guarded(n=4 * npix)
    qbuf, qv = guarded(n=want_q.size)
    F._chk(lib.stem_nchw3_to_nhwc4(xd.data_ptr(), yv.data_ptr(), B, H, W, qv.data_ptr(), F._stream()))
    torch.cuda.synchronize()
    assert np.array_equal(bits(yv), want_y.reshape(-1).view(np.uint32)) and guards_intact(ybuf, yv)
    assert np.array_equal(bits(qv), want_q.view(np.uint32)), (host(qv), want_q)
    assert guards_intact(qbuf, qv)
    assert ref.amax_record_max(host(qv)) == ((npix + 1023) // 1024, 123.5)
    out = F.nchw3_to_nhwc4(xd)
    assert np.array_equal(host(out), want_y) and np.array_equal(bits(out._stem_q), want_q.view(np.uint32))
    ybuf, yv = guarded(n=4 * npix)                                  # without a record: the same pixels
    F._chk(lib.stem_nchw3_to_nhwc4(xd.data_ptr(), yv.data_ptr(), B, H, W, 0, F._stream()))
    torch.cuda.synchronize()
    assert np.array_equal(bits(yv), want_y.reshape(-1).view(np.uint32)) and guards_intact(ybuf, yv)


@pytest.fixture(scope="module")
def amax_input():
    """the largest tensor of this file (70000 x 104 floats), drawn once: every amax case is a corner of it"""
    rng = np.random.default_rng(31)
    return ((rng.random((70000, 104), dtype=np.float32) - 0.5) * 10.0 ** rng.uniform(-2, 1, (70000, 1)).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("case", ref.AMAX_CASES, ids=lambda c: "npix%d_C%d_slots%d" % c)
def test_amax_nhwc(F, lib, amax_input, case):
    """max |x| of an NHWC tensor with pitch C + 4 (1e30 in the pitch columns: one of them read shows), max_slots below and above the
    natural count of one workgroup per 2048 float4 pieces: the slot count is the entry point's, the maximum over the slots is
    max |x| exactly, every slot is a maximum of part of the tensor (0 <= slot <= max), words 2..15 are zero, nothing behind the slots
    is written; an all-zero tensor gives 0"""
    npix, C, max_slots = case
    a = amax_input[:npix, :C].copy()
    a[npix // 3, C - 1] = -77.25                                    # the maximum in the last channel, in one slot only
    x = torch.full((npix, C + 4), 1e30, dtype=torch.float32, device="cuda")
    x[:, :C] = dev(a)
    ns = ref.amax_slots(npix, C, max_slots)
    for data, want_max in ((x, 77.25), (torch.zeros_like(x), 0.0)):
        if want_max == 0.0:
            data[:, C:] = 1e30
        qbuf, qv = guarded(n=ref.QREC_HDR + ns)
        F._chk(lib.stem_amax_nhwc(data.data_ptr(), C + 4, npix, C, qv.data_ptr(), max_slots, F._stream()))
        torch.cuda.synchronize()
        q = host(qv)
        assert ref.amax_record_max(q) == (ns, want_max) and float(np.abs(a).max()) == 77.25
        assert not q[2:ref.QREC_HDR].view(np.uint32).any() and guards_intact(qbuf, qv)
        slots = q[ref.QREC_HDR:]
        assert (slots >= 0).all() and (slots <= want_max).all() and (slots == want_max).sum() == (1 if want_max else ns)
