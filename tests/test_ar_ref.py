"""CPU: pins tests/ar_ref.py, the float32 emulation of the coding loop's canonical product and the raster-order encoder built on it,
before tests/test_hip_ar_ops.py holds the HIP kernels to it bit for bit.  The emulation is compared with float64 under a bound derived
from the count of roundings, shown to differ from other summation orders, and checked at constructed ties; the raster-order loop is
compared with a teacher-forced float64 evaluation whose context is the masked convolution itself."""
import numpy as np
import pytest

import ar_ref as ar
from conftest import assert_close

U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the product
@pytest.mark.parametrize("n", [96, 260, 516, 768, 1024])
def test_gemv3_vs_float64(n):
    """|gemv3 - gemv3_f64| <= d u / (1 - d u) (sum |x w| + |bias|), u = 2^-24, d = the roundings on the longest path (4 per step + the
    steps + 6 + 1: 12, 17, 22, 22, 27 for these lengths); derived, not measured.  Measured max |err| / (u mag) over 38 rows: 0.43 (96),
    0.24 (260), 0.27 (516), 0.16 (768), 0.20 (1024) against d = 12 .. 27.  The result differs from numpy's float32 dot on 25, 28, 32,
    29, 33 of the 38 rows and from a sequential float32 sum on 30, 36, 33, 34, 34: the order is exercised, a kernel that strays from
    it cannot pass by luck."""
    W, bias, xs, woffs = ar.product_case((n,), 38, seed=n)
    segs = list(zip(xs, woffs))
    y = ar.gemv3(W, bias, segs)
    exact, mag = ar.gemv3_f64(W, bias, segs)
    d = ar.gemv3_depth(segs)
    assert d == 5 * -(-n // 256) + 7
    ratio = np.abs(y.astype(np.float64) - exact) / (U * mag)
    print(f"[gemv3 vs f64] len {n}: max |err| / (u mag) = {ratio.max():.2f}, depth {d}")
    assert (np.abs(y.astype(np.float64) - exact) <= d * U / (1 - d * U) * mag).all()
    cols = W[:, woffs[0]:woffs[0] + n]
    blas = cols @ xs[0] + bias
    seq = np.zeros(38, np.float32)
    for k in range(n):
        seq = seq + cols[:, k] * xs[0][k]
    seq = seq + bias
    print(f"[gemv3 order] len {n}: {int((y != blas).sum())} of 38 rows differ from np.dot, {int((y != seq).sum())} from a sequential sum")
    assert blas.dtype == np.float32 and (y != blas).any() and (y != seq).any()


@pytest.mark.parametrize("lens", ar.SEGMENT_SETS)
def test_gemv3_segments_batch_and_activation(lens):
    """several segments at scattered weight columns against float64 under the same bound; a batch of inputs gives each input's own
    result; LeakyReLU is v > 0 ? v : v * slope on the same sum; a null bias adds nothing"""
    W, bias, xs, woffs = ar.product_case(lens, 6, seed=sum(lens))
    segs = list(zip(xs, woffs))
    y = ar.gemv3(W, bias, segs)
    exact, mag = ar.gemv3_f64(W, bias, segs)
    d = ar.gemv3_depth(segs)
    assert (np.abs(y.astype(np.float64) - exact) <= d * U / (1 - d * U) * mag).all()
    assert (y > 0).any() and (y < 0).any()
    assert np.array_equal(ar.gemv3(W, bias, segs, ar.ACT_LRELU, ar.SLOPE), np.where(y > 0, y, y * np.float32(ar.SLOPE)))
    y0 = ar.gemv3(W, None, segs)
    assert np.array_equal(y0 + bias, y)
    xs2 = [np.stack([x, -x[::-1], 0.5 * x]) for x in xs]
    yb = ar.gemv3(W, bias, list(zip(xs2, woffs)))
    assert yb.shape == (3, 6)
    for b in range(3):
        assert np.array_equal(yb[b], ar.gemv3(W, bias, [(x[b], o) for x, o in zip(xs2, woffs)]))


def test_gemv3_single_terms_are_exact():
    """a row with a single 1.0 returns the input it selects, whichever lane and step holds it (0 + x and x + 0 are exact): the
    construction of the index ties in tests/test_hip_ar_ops.py"""
    x = np.arange(1, 521, dtype=np.float32) / np.float32(7)
    W = np.zeros((5, 520), np.float32)
    cols = [0, 3, 255, 256, 519]
    W[np.arange(5), cols] = 1.0
    assert np.array_equal(ar.gemv3(W, None, [(x, 0)]), x[cols])


# ---------------------------------------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("name,hw,G", ar.IMAGE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_encode_image_vs_float64(name, hw, G):
    """The raster-order float32 loop against gp_f64_forced on its own final buffer: gp within the project's gate (1e-4, floor 0.1);
    sym and idx equal the float64 ones except near ties (float64 y - mu within 1e-4 of a half-integer; float64 scale within 1e-4
    relative of a table entry or of the bound), of which a case may hold at most 1%.  Measured near-tie share per image: 0 in nets A and B up to (4, 6) and in
    net C; 1 of 384 in A (3, 16), 1 of 140 in B (7, 5) (0.71%, the largest), 1 of 192 in B (3, 16), 1 of 1040 in D (2, 5), at most 3 of
    3456 in A (12, 36); no mismatch outside them; max |gp32 - gp64| = 8.4e-7.  The symbols leave
    -4 .. 4 and the indexes take at least three values: the draws are not trivial."""
    net = ar.net(name)
    target, hp, tp = ar.case_inputs(name, hw, G)
    ref = ar.reference(name, hw, G)
    H, W = hw
    M = net["M"]
    table = np.asarray(ar.TABLE, np.float32).astype(np.float64)
    worst = 0.0
    for g in range(G):
        gp64 = ar.gp_f64_forced(net, ref["buf"][g], hp[g], None if tp is None else tp[g])
        assert_close(ref["gp"][g], gp64, 1e-4, what=f"{name} {hw} image {g} gp", floor=0.1)
        worst = max(worst, float(np.abs(ref["gp"][g] - gp64).max()))
        s64, mu64 = gp64[:, :M], gp64[:, M:]
        d = target[g].reshape(H * W, M).astype(np.float64) - mu64
        near = np.abs(np.abs(d - np.floor(d)) - 0.5) < 1e-4
        edges = np.concatenate([table[:-1], [float(np.float32(ar.BOUND))]])
        near |= (np.abs(s64[..., None] - edges) <= 1e-4 * edges).any(-1)
        print(f"[near ties] {name} {hw} image {g}: {int(near.sum())} of {near.size}")
        assert near.mean() <= 0.01
        assert np.array_equal(ref["sym"][g][~near], np.rint(d).astype(np.int32)[~near])
        assert np.array_equal(ref["idx"][g][~near], ar.index_direct(s64, ar.TABLE)[~near])
        # the buffer is the quantised target on a ring of zeros
        inner = ref["buf"][g][2:2 + H, 2:2 + W].reshape(H * W, M)
        assert np.array_equal(inner, ref["sym"][g].astype(np.float32) + ref["gp"][g][:, M:])
        ring = ref["buf"][g].copy()
        ring[2:2 + H, 2:2 + W] = 0
        assert not ring.any()
    print(f"[gp32 vs gp64] {name} {hw}: max |diff| = {worst:.2e}")
    sym, idx = ref["sym"], ref["idx"]
    assert sym.min() < -4 and sym.max() > 4 and idx.min() == 0
    if H * W >= 3:
        assert len(np.unique(idx)) >= 3


def test_encode_image_is_encode_images_per_image():
    name, hw, G = "A", (4, 6), 3
    target, hp, tp = ar.case_inputs(name, hw, G)
    ref = ar.reference(name, hw, G)
    for g in range(G):
        sym, idx, buf, gp = ar.encode_image(ar.net(name), target[g], hp[g], tp[g])
        assert all(np.array_equal(a, ref[k][g]) for a, k in ((sym, "sym"), (idx, "idx"), (buf, "buf"), (gp, "gp")))
    assert not np.array_equal(ref["sym"][0], ref["sym"][1])
    # image g does not depend on how many are drawn with it
    assert np.array_equal(ar.case_inputs(name, hw, 1)[0][0], target[0])


# ---------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("table", ar.INDEX_TABLES, ids=lambda t: f"T{len(t)}")
def test_index_at_the_table_entries(table):
    """index == T - 1 - #{t < T - 1 : max(s, bound) <= table[t]} at every entry, its float32 neighbours, the bound and its
    neighbours, 0, -1 and 1e9; an entry itself belongs to the interval BELOW it, its upper neighbour to the one above"""
    s = ar.index_scales(table)
    T = len(table)
    t32 = np.asarray(table, np.float32)
    want = np.array([T - 1 - sum(1 for t in range(T - 1) if max(v, np.float32(ar.BOUND)) <= t32[t]) for v in s], np.int32)
    got = ar.index(s, table)
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(ar.index_direct(s, table), want)
    assert np.array_equal(got[:T], np.minimum(np.arange(T), T - 1))               # s == table[k]: k entries are below it
    assert np.array_equal(got[T:2 * T], np.minimum(np.arange(T) + 1, T - 1))      # just above table[k]
    assert got[-1] == T - 1 and got[-2] == 0 and got[-3] == 0                     # 1e9, -1, 0
    assert np.array_equal(got[3 * T:3 * T + 3], [0, min(1, T - 1), 0])            # the bound is the first entry


def test_finish_encode_rounds_ties_to_even():
    """mu = 0.25, pix = k + 0.75: pix - mu = k + 1/2 exactly, k = -4 .. 3 -> -4 -2 -2 0 0 2 2 4; pix - mu = +-0.25 -> 0;
    pix' = q + mu in float32; finish_decode(sym) gives the same pixel"""
    M = len(ar.TIE_PIX)
    gp = np.concatenate([np.full(M, 1.0, np.float32), np.full(M, ar.TIE_MU, np.float32)])
    pix = np.array(ar.TIE_PIX, np.float32)
    assert np.array_equal((pix - gp[M:])[:8], np.arange(-4, 4) + np.float32(0.5))
    sym, idx, out = ar.finish_encode(gp, pix, ar.TABLE)
    assert sym.dtype == np.int32 and np.array_equal(sym, ar.TIE_SYM)
    assert np.array_equal(out, np.array(ar.TIE_SYM, np.float32) + np.float32(ar.TIE_MU)) and out.dtype == np.float32
    assert np.array_equal(idx, np.full(M, 3)) and np.array_equal(ar.finish_decode(gp, sym), out)


@pytest.mark.parametrize("M", [4, 52, 260])
def test_finish_case_covers_scales_and_ties(M):
    starts = range(0, 60, 4) if M == 4 else (0,)
    seen_s, seen_t = set(), set()
    for start in starts:
        gp, pix, tie = ar.finish_case(M, ar.TABLE, 1, start)
        assert gp.shape == (1, 2 * M) and pix.shape == (1, M) and gp.dtype == np.float32 and pix.dtype == np.float32
        seen_s |= set(gp[0, :M].tolist())
        seen_t |= set((pix - gp[:, M:])[tie].tolist())
    assert seen_s == set(ar.index_scales(ar.TABLE).tolist()) and len(seen_s) == 27        # the bound is the first entry
    assert seen_t == {k + 0.5 for k in range(-4, 4)} | {0.25, -0.25}


# ---------------------------------------------------------------------------------------------------------------- order and pack
@pytest.mark.parametrize("hw", ar.WAVE_GEOMETRIES + ((1, 2), (2, 2)))
def test_wave_range_partitions_the_grid_in_dependency_order(hw):
    """the positions of steps 0 .. W + 3(H-1) - 1 are every position of the H x W grid exactly once, and all twelve context
    neighbours of a position (rows h-2, h-1 at columns w-2 .. w+2, row h at w-2, w-1) that lie inside the grid belong to EARLIER steps;
    the steps agree with codec.wave_order"""
    from spatiotemporalentropymodel_amd.codec import wave_order
    H, W = hw
    step = {}
    seq = []
    for t in range(W + 3 * (H - 1)):
        h0, n = ar.wave_range(t, H, W)
        for h in range(h0, h0 + n):
            w = t - 3 * h
            assert 0 <= h < H and 0 <= w < W and (h, w) not in step
            step[(h, w)] = t
            seq.append(h * W + w)
    assert len(step) == H * W and max(step.values()) == W + 3 * (H - 1) - 1
    assert max(ar.wave_range(t, H, W)[1] for t in range(W + 3 * (H - 1))) == min(H, (W + 2) // 3)
    for (h, w), t in step.items():
        for dh, dw in [(-2, d) for d in range(-2, 3)] + [(-1, d) for d in range(-2, 3)] + [(0, -2), (0, -1)]:
            if (h + dh, w + dw) in step:
                assert step[(h + dh, w + dw)] < t
    assert np.array_equal(wave_order(H, W)[0], seq)


@pytest.mark.parametrize("K,C", [(8, 4), (104, 52)])
def test_pack_ctx_vs_explicit_indexing(K, C):
    w = np.random.default_rng(K).standard_normal((K, C, 5, 5)).astype(np.float32)
    out = ar.pack_ctx(w)
    assert out.shape == (K, 12, C) and out.flags["C_CONTIGUOUS"]
    taps = [(r, c) for r in range(5) for c in range(5)][:12]
    assert taps[-1] == (2, 1) and all(ar.MASK_A[r, c] == 1 for r, c in taps) and ar.MASK_A.sum() == 12
    for t, (r, c) in enumerate(taps):
        assert np.array_equal(out[:, t, :], w[:, :, r, c])


def test_nets_and_cases():
    """the tables both test files iterate over: widths that reach the second, third and fourth 256-column step with one or two live
    lanes, a row count that is no multiple of 16, and scales on both sides of the bound"""
    for name, (M, n0, n1, has_tp) in ar.NETS.items():
        net = ar.net(name)
        assert net["w_ctx"].shape == (2 * M, 12 * M) and net["w0"].shape == (n0, (6 if has_tp else 4) * M) and net["w2"].shape == (2 * M, n1)
        assert all(v % 4 == 0 for v in (M, n0, n1)) and 5 * M <= 1024 and n0 <= 1024 and n1 <= 1024
        assert net["b2"][0] < ar.BOUND < net["b2"][1]
    assert 5 * ar.NETS["C"][0] == 260 and ar.NETS["C"][1] == 264 and (2 * ar.NETS["C"][0]) % 16 != 0
    assert ar.NETS["D"][1] == 3 * 256 + 4 and 5 * ar.NETS["D"][0] == 520
