"""GPU, op level: every kernel form of the coding loop's product and every kernel that calls its scale-to-index search and its
quantisation (csrc/ar.hip, csrc/ar_persistent.hip; the arithmetic itself is csrc/ar_canon.h) against tests/ar_ref.py, the numpy statement of the canonical product of include/stem_ar_batch.h, which
tests/test_ar_ref.py pins on the CPU.  Every comparison is of bits.  Outputs are allocated with a sentinel and whatever a call does
not own must keep it: rows >= N, the ring of the latent buffer, symbols and indexes of other images.  Mailboxes the codec keeps in
pinned host memory are pinned here.

The whole-image encoders are compared with the raster-order reference loop; the decoders decode the host coder's strings of the
REFERENCE's symbols and indexes, so a decoder that strays from the canonical floats by a bit leaves another buffer or runs out of
sync with its string."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ar_ref as ar
from test_hip_wave_order import SLOPE, TABLE, _host_string, _tables, _words_left

assert tuple(TABLE) == ar.TABLE and SLOPE == ar.SLOPE          # _tables() codes with that table

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

SENT = -777.25                 # float sentinel
ISENT = -12345                 # int32 sentinel
NAN = float("nan")


def _dev():
    return torch.device("cuda:0")


def D(a):
    """a numpy array -> a device tensor of its own (256-byte aligned)"""
    return torch.from_numpy(np.array(a, copy=True)).to(_dev()).contiguous()


def full(shape, value, dtype=torch.float32, pinned=False):
    t = torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype)
    return t.pin_memory() if pinned else t.to(_dev())


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    view = np.uint32 if got.dtype == np.float32 else got.dtype
    bad = got.view(view) != want.view(view)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]!r} vs {want[tuple(np.argwhere(bad)[0])]!r}"


@pytest.fixture(scope="module")
def hip():
    from spatiotemporalentropymodel_amd import _lib, functional as F
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.hip(), F


def _last_error(lib):
    return (lib.stem_last_error() or b"").decode()


def _seg_args(xs, lens, woffs):
    """the nine segment arguments of stem_gemv3 / stem_gemv3_decode: an empty segment has a null base"""
    out = []
    for i in range(3):
        if i < len(lens):
            out += [xs[i].data_ptr() if lens[i] else None, lens[i], woffs[i]]
        else:
            out += [None, 0, 0]
    return out


# =========================================================================================================== single products
@pytest.mark.parametrize("lens", ar.SEGMENT_SETS, ids=str)
@pytest.mark.parametrize("N", ar.PRODUCT_ROWS)
def test_gemv3_and_gemv3_wave_vs_reference(hip, N, lens):
    """stem_gemv3, and stem_gemv3_wave for step 6 of a 4 x 6 grid (two positions; its first segment addressed by the position's row
    and column, the others by its rank in the step), with and without bias and LeakyReLU, rows of both signs; weight columns with
    gaps, not ascending, ldw larger than what the segments use; y[N:] and the rows of other positions keep the sentinel"""
    lib, F = hip
    st = F._stream()
    W, bias, xs, woffs = ar.product_case(lens, N, seed=1000 * N + sum(lens))
    Wd, bd, xd = D(W), D(bias), [D(x) for x in xs]
    ref_plain = ar.gemv3(W, bias, list(zip(xs, woffs)))
    if N >= 3:
        assert (ref_plain > 0).any() and (ref_plain < 0).any()
    for b_np, b_dev in ((bias, bd), (None, None)):
        for act in (ar.ACT_NONE, ar.ACT_LRELU):
            what = f"gemv3 N={N} lens={lens} bias={b_np is not None} act={act}"
            y = full(N + 5, SENT)
            F._chk(lib.stem_gemv3(Wd.data_ptr(), W.shape[1], b_dev.data_ptr() if b_dev is not None else None, *_seg_args(xd, lens, woffs),
                                  y.data_ptr(), N, act, ar.SLOPE, st))
            y = host(y)
            same(y[:N], ar.gemv3(W, b_np, list(zip(xs, woffs)), act, ar.SLOPE), what)
            same(y[N:], np.full(5, SENT, np.float32), what + " tail")
    # the wavefront form: H x W = 4 x 6, step 6 = positions (1, 3) and (2, 0)
    H, Wg, t = 4, 6, 6
    h0, npos = ar.wave_range(t, H, Wg)
    assert (h0, npos) == (1, 2)
    npmax = min(H, (Wg + 2) // 3)
    rng = np.random.default_rng(N + sum(lens))
    grids = [rng.standard_normal((H, Wg, n) if i == 0 else (npmax, n)).astype(np.float32) for i, n in enumerate(lens)]
    gd = [D(g) if g.size else None for g in grids]
    from spatiotemporalentropymodel_amd._lib import WaveSeg as S
    segs = (S * 3)()
    for i, n in enumerate(lens):
        segs[i] = S(gd[i].data_ptr() if n else None, n, woffs[i], Wg * n if i == 0 else 0, n if i == 0 else 0, 0 if i == 0 else n)
    ldy = N + 3
    for b_np, b_dev in ((bias, bd), (None, None)):
        for act in (ar.ACT_NONE, ar.ACT_LRELU):
            y = full((npmax + 1, ldy), SENT)
            F._chk(lib.stem_gemv3_wave(Wd.data_ptr(), W.shape[1], b_dev.data_ptr() if b_dev is not None else None, C.addressof(segs), y.data_ptr(), ldy, N,
                                       act, ar.SLOPE, t, H, Wg, st))
            y = host(y)
            want = np.full((npmax + 1, ldy), SENT, np.float32)
            for p in range(npos):
                h = h0 + p
                want[p, :N] = ar.gemv3(W, b_np, [(g[h, t - 3 * h] if i == 0 else g[p], woffs[i]) for i, g in enumerate(grids)], act, ar.SLOPE)
            same(y, want, f"gemv3_wave N={N} lens={lens} bias={b_np is not None} act={act}")


@pytest.mark.parametrize("lens", ar.SEGMENT_SETS, ids=str)
@pytest.mark.parametrize("N", ar.PRODUCT_ROWS)
def test_gemv3_decode_plain_product_vs_reference(hip, N, lens):
    """stem_gemv3_decode without write-back and without a table is the same product: the row counts, segment sets, bias present and
    null, no activation and LeakyReLU of the stem_gemv3 test (the kernel has its own exit at n >= N); y[N:] keeps the sentinel"""
    lib, F = hip
    W, bias, xs, woffs = ar.product_case(lens, N, seed=77 * N + sum(lens))
    Wd, bd, xd = D(W), D(bias), [D(x) for x in xs]
    for b_np, b_dev in ((bias, bd), (None, None)):
        for act in (ar.ACT_NONE, ar.ACT_LRELU):
            what = f"gemv3_decode N={N} lens={lens} bias={b_np is not None} act={act}"
            y = full(N + 5, SENT)
            F._chk(lib.stem_gemv3_decode(Wd.data_ptr(), W.shape[1], b_dev.data_ptr() if b_dev is not None else None, *_seg_args(xd, lens, woffs),
                                         y.data_ptr(), N, act, ar.SLOPE, None, None, None, 4, 0, None, 0, 0.0, None, F._stream()))
            y = host(y)
            same(y[:N], ar.gemv3(W, b_np, list(zip(xs, woffs)), act, ar.SLOPE), what)
            same(y[N:], np.full(5, SENT, np.float32), what + " tail")


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_gemv3_decode_write_back_and_substitution(hip, name):
    """the context product of nets A, C, D (2M rows over 5M | 5M | 2M floats).  The previous position's symbols sit in a pinned
    mailbox: pix_prev <- sym + mean (M floats, the next ones keep the sentinel).  prev_is_left = 1: the second half of segment 2 is
    sym + mean whatever memory holds -- it holds NaN, so reading it shows; prev_is_left = 0: memory is read."""
    lib, F = hip
    net = ar.net(name)
    M = net["M"]
    P = 2 * M
    rng = np.random.default_rng(M)
    x0, x1 = (rng.standard_normal(5 * M).astype(np.float32) for _ in range(2))
    x2 = rng.standard_normal(P).astype(np.float32)
    sym = rng.integers(-9, 10, M).astype(np.int32)
    mean = rng.standard_normal(M).astype(np.float32)
    prev = ar.finish_decode(np.concatenate([mean, mean]), sym)
    Wd, bd = D(net["w_ctx"]), D(net["b_ctx"])
    sym_box = torch.from_numpy(sym.copy()).pin_memory()
    mean_d = D(mean)
    for left in (1, 0):
        x2_mem = x2.copy()
        if left:
            x2_mem[M:] = NAN
        xd = [D(x0), D(x1), D(x2_mem)]
        y, pix = full(P + 4, SENT), full(M + 4, SENT)
        F._chk(lib.stem_gemv3_decode(Wd.data_ptr(), 12 * M, bd.data_ptr(), xd[0].data_ptr(), 5 * M, 0, xd[1].data_ptr(), 5 * M, 5 * M,
                                     xd[2].data_ptr(), P, 10 * M, y.data_ptr(), P, 0, 0.0, sym_box.data_ptr(), mean_d.data_ptr(), pix.data_ptr(), M, left,
                                     None, 0, 0.0, None, F._stream()))
        y, pix = host(y), host(pix)
        seg2 = np.concatenate([x2[:M], prev]) if left else x2
        what = f"net {name} prev_is_left={left}"
        same(y[:P], ar.gemv3(net["w_ctx"], net["b_ctx"], [(x0, 0), (x1, 5 * M), (seg2, 10 * M)]), what)
        same(y[P:], np.full(4, SENT, np.float32), what + " y tail")
        same(pix, np.concatenate([prev, np.full(4, SENT, np.float32)]), what + " pix_prev")
        same(host(xd[2]), x2_mem, what + " segment 2 in memory")


@pytest.mark.parametrize("table", ar.INDEX_TABLES, ids=lambda t: f"T{len(t)}")
def test_gemv3_decode_index_epilogue_at_ties(hip, table):
    """rows with a single 1.0 and no bias return the input they select exactly, wherever it sits in the 516-float segment: every table
    entry, its neighbours, the bound and its neighbours, 0, -1 and 1e9 arrive as scales and the epilogue's search must give
    ar_ref.index; rows >= M get no index and the mailbox's tail keeps the sentinel"""
    lib, F = hip
    s = ar.index_scales(table)
    M = -(-len(s) // 4) * 4
    N, n = M + 8, 516
    rng = np.random.default_rng(len(table))
    x = rng.standard_normal(n).astype(np.float32)
    special = [515, 512, 256, 260, 255, 252, 0, 3, 511, 4]                       # the first and last lanes of each 256-column step
    cols = np.array(special + [c for c in ((np.arange(n) * 37 + 7) % n).tolist() if c not in special][:M - len(special)])
    assert len(set(cols.tolist())) == M == len(cols)
    scales = np.concatenate([s, np.full(M - len(s), 0.3, np.float32)])
    x[cols] = scales
    W = np.zeros((N, n + 12), np.float32)
    W[np.arange(M), 4 + cols] = 1.0
    W[M:, 4:4 + n] = rng.standard_normal((N - M, n)).astype(np.float32) / 23
    ref_y = ar.gemv3(W, None, [(x, 4)])
    same(ref_y[:M], scales, "the construction")
    T = len(table)
    Wd, xd, td = D(W), D(x), D(np.asarray(table, np.float32))
    for bias in (None, D(np.zeros(N, np.float32))):
        y = full(N + 4, SENT)
        idx = full(M + 4, ISENT, torch.int32, pinned=True)
        F._chk(lib.stem_gemv3_decode(Wd.data_ptr(), n + 12, bias.data_ptr() if bias is not None else None, xd.data_ptr(), n, 4, None, 0, 0, None, 0, 0,
                                     y.data_ptr(), N, 0, 0.0, None, None, None, M, 0, td.data_ptr(), T, ar.BOUND,
                                     idx.data_ptr(), F._stream()))
        y = host(y)
        same(y[:N], ref_y, "scales")
        same(idx.numpy(), np.concatenate([ar.index(scales, table), np.full(4, ISENT, np.int32)]), f"indexes T={T}")


# =========================================================================================================== finish and index kernels
FINISH_CASES = [(M, start) for M, starts in ((4, range(0, 60, 4)), (52, (0,)), (260, (0,))) for start in starts]


@pytest.mark.parametrize("table", ar.INDEX_TABLES, ids=lambda t: f"T{len(t)}")
@pytest.mark.parametrize("M,start", FINISH_CASES)
def test_finish_and_index_kernels_vs_reference(hip, M, start, table):
    """stem_ar_finish_encode, stem_ar_index and stem_ar_finish_decode on entropy parameters given directly: scales at every table entry,
    its float32 neighbours, the bound and its neighbours, 0, -1, 1e9; pixels at exact half-integer ties (to even) and at +-0.25 of the
    mean.  M = 260 spans two workgroups of 256 threads; M = 4 walks the lists four elements at a time."""
    lib, F = hip
    st = F._stream()
    gp, pix, tie = ar.finish_case(M, table, 1, start)
    gp, pix = gp[0], pix[0]
    sym_r, idx_r, pix_r = ar.finish_encode(gp, pix, table)
    if M == 260:
        assert set(sym_r[tie[0]].tolist()) == {-4, -2, 0, 2, 4}
    T = len(table)
    gd, td = D(gp), D(np.asarray(table, np.float32))
    tail_f, tail_i = np.full(4, SENT, np.float32), np.full(4, ISENT, np.int32)
    pd = D(np.concatenate([pix, tail_f]))
    sym, idx = (full(M + 4, ISENT, torch.int32) for _ in range(2))
    F._chk(lib.stem_ar_finish_encode(gd.data_ptr(), td.data_ptr(), T, ar.BOUND, pd.data_ptr(), sym.data_ptr(), idx.data_ptr(), M, st))
    same(host(sym), np.concatenate([sym_r, tail_i]), "finish_encode sym")
    same(host(idx), np.concatenate([idx_r, tail_i]), "finish_encode idx")
    same(host(pd), np.concatenate([pix_r, tail_f]), "finish_encode pix")
    same(host(gd), gp, "gp is read only")
    idx2 = full(M + 4, ISENT, torch.int32, pinned=True)
    F._chk(lib.stem_ar_index(gd.data_ptr(), td.data_ptr(), T, ar.BOUND, idx2.data_ptr(), M, st))
    torch.cuda.synchronize()
    same(idx2.numpy(), np.concatenate([idx_r, tail_i]), "ar_index")
    pd2 = full(M + 4, SENT)
    sym_box = torch.from_numpy(sym_r.copy()).pin_memory()
    F._chk(lib.stem_ar_finish_decode(gd.data_ptr(), sym_box.data_ptr(), pd2.data_ptr(), M, st))
    same(host(pd2), np.concatenate([ar.finish_decode(gp, sym_r), tail_f]), "finish_decode")
    same(ar.finish_decode(gp, sym_r), pix_r, "the decoder's pixel is the encoder's")


@pytest.mark.parametrize("table", ar.INDEX_TABLES, ids=lambda t: f"T{len(t)}")
@pytest.mark.parametrize("M", (4, 52, 260))
def test_finish_encode_wave_vs_reference(hip, M, table):
    """stem_ar_finish_encode_wave on step 15 of a 6 x 16 grid: six positions (6 M > 256 threads for M = 52 and 260), the same scales
    and ties; the pixels, symbols and indexes of every other position and the ring of the buffer keep the sentinel"""
    lib, F = hip
    H, W, t = 6, 16, 15
    h0, npos = ar.wave_range(t, H, W)
    assert (h0, npos) == (0, 6) and npos == min(H, (W + 2) // 3)
    gp, pix, _ = ar.finish_case(M, table, npos)
    sym_r, idx_r, pix_r = ar.finish_encode(gp, pix, table)
    buf = np.full((H + 4, W + 4, M), SENT, np.float32)
    want_buf, want_sym, want_idx = buf.copy(), np.full((H * W, M), ISENT, np.int32), np.full((H * W, M), ISENT, np.int32)
    for p in range(npos):
        h, w = h0 + p, t - 3 * (h0 + p)
        buf[h + 2, w + 2] = pix[p]
        want_buf[h + 2, w + 2], want_sym[h * W + w], want_idx[h * W + w] = pix_r[p], sym_r[p], idx_r[p]
    bd, gd, td = D(buf), D(gp), D(np.asarray(table, np.float32))
    sym, idx = (full((H * W, M), ISENT, torch.int32) for _ in range(2))
    F._chk(lib.stem_ar_finish_encode_wave(gd.data_ptr(), td.data_ptr(), len(table), ar.BOUND, bd.data_ptr(),
                                          sym.data_ptr(), idx.data_ptr(), M, t, H, W, W + 4, 2, F._stream()))
    same(host(bd), want_buf, "buf")
    same(host(sym), want_sym, "sym")
    same(host(idx), want_idx, "idx")


@pytest.mark.parametrize("K,Cn", [(8, 4), (104, 52)])
def test_pack_ctx_gemv_vs_reference(hip, K, Cn):
    lib, F = hip
    w = np.random.default_rng(K).standard_normal((K, Cn, 5, 5)).astype(np.float32)
    out, wd = full(K * 12 * Cn + 8, SENT), D(w)
    F._chk(lib.stem_pack_ctx_gemv(wd.data_ptr(), out.data_ptr(), K, Cn, F._stream()))
    same(host(out), np.concatenate([ar.pack_ctx(w).reshape(-1), np.full(8, SENT, np.float32)]), f"pack_ctx {K} x {Cn}")


# =========================================================================================================== whole images
@functools.lru_cache(maxsize=None)
def _net(name):
    """a net of ar_ref on the device, with the argument lists every stem_ar_* image call begins with"""
    n = ar.net(name)
    d = {k: D(v) for k, v in n.items() if isinstance(v, np.ndarray)}
    M, n0, n1 = n["M"], n["n0"], n["n1"]
    d["args"] = (d["w_ctx"].data_ptr(), 12 * M, d["b_ctx"].data_ptr(), d["w0"].data_ptr(), n["w0"].shape[1], d["b0"].data_ptr(), n0,
                 d["w1"].data_ptr(), n0, d["b1"].data_ptr(), n1, d["w2"].data_ptr(), n1, d["b2"].data_ptr())
    d["table_args"] = (d["table"].data_ptr(), len(ar.TABLE), ar.BOUND, ar.SLOPE)
    d.update(M=M, n0=n0, n1=n1)
    return d


def _device_inputs(name, hw, G):
    target, hp, tp = ar.case_inputs(name, hw, G)
    return target, D(hp), D(tp) if tp is not None else None


def _padded(target, extra=1):
    """[G, H, W, M] -> [G + extra, H + 4, W + 4, M] on the device: the targets on a ring of zeros, then images of sentinels"""
    G, H, W, M = target.shape
    buf = np.zeros((G + extra, H + 4, W + 4, M), np.float32)
    buf[:G, 2:2 + H, 2:2 + W] = target
    buf[G:] = SENT
    return D(buf)


def _want(ref, key, G, extra=1):
    a = ref[key][:G]
    return np.concatenate([a, np.full((extra,) + a.shape[1:], SENT if a.dtype == np.float32 else ISENT, a.dtype)])


ENCODE_IMAGE_CASES = [c for c in ar.IMAGE_CASES if c[2] == 3]


@pytest.mark.parametrize("name,hw,Gn", ENCODE_IMAGE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_encode_image_vs_reference(hip, name, hw, Gn):
    """stem_ar_encode_image, image by image, against the raster-order reference loop: sym, idx and the returned buf bit for bit; the
    images it was not given keep their sentinels"""
    lib, F = hip
    net, ref = _net(name), ar.reference(name, hw, Gn)
    H, W = hw
    M, P = net["M"], 2 * net["M"]
    target, hp, tp = _device_inputs(name, hw, Gn)
    npmax = min(H, (W + 2) // 3)
    scratch = [full((npmax, n), NAN) for n in (P, net["n0"], net["n1"], P)]
    for g in range(Gn):
        buf = _padded(target)
        sym, idx = (full((Gn + 1, H * W, M), ISENT, torch.int32) for _ in range(2))
        F._chk(lib.stem_ar_encode_image(*net["args"], buf[g].data_ptr(), H, W, M, 2, tp[g].data_ptr() if tp is not None else None, hp[g].data_ptr(),
                                        *[t.data_ptr() for t in scratch], *net["table_args"], sym[g].data_ptr(), idx[g].data_ptr(), F._stream()))
        got_buf, got_sym, got_idx = host(buf), host(sym), host(idx)
        what = f"encode_image {name} {hw} image {g}"
        same(got_sym[g], ref["sym"][g], what + " sym")
        same(got_idx[g], ref["idx"][g], what + " idx")
        same(got_buf[g], ref["buf"][g], what + " buf")
        others = [i for i in range(Gn + 1) if i != g]
        assert (got_sym[others] == ISENT).all() and (got_idx[others] == ISENT).all(), what + ": another image's symbols were written"
        same(got_buf[others], host(_padded(target))[others], what + " other images")


ENCODE_BATCH_CASES = [(n, hw, G) for n, hw, Gn in ar.IMAGE_CASES for G in ((1, 3) if Gn == 3 else (Gn,))]


@pytest.mark.parametrize("name,hw,G", ENCODE_BATCH_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_encode_batch_vs_reference(hip, name, hw, G):
    """stem_ar_encode_batch for G = 1 and 3 (register tiles of one and two positions, workgroups with idle wavefronts on net C), and
    for nine 12 x 36 images of net A: 108 positions in the widest step, more than three times the 32 workgroup rows, so the four-wide,
    two-wide and single tiles all run.  Per image: the reference's sym, idx and buf, bit for bit."""
    lib, F = hip
    Gn = next(c[2] for c in ar.IMAGE_CASES if c[0] == name and c[1] == hw)
    net, ref = _net(name), ar.reference(name, hw, Gn)
    H, W = hw
    M, P = net["M"], 2 * net["M"]
    target, hp, tp = _device_inputs(name, hw, Gn)
    if G == 9:
        assert G * min(H, (W + 2) // 3) > 3 * 32
    npmax = min(H, (W + 2) // 3)
    scratch = [full((G, npmax, n), NAN) for n in (P, net["n0"], net["n1"], P)]
    buf = _padded(target[:G])
    sym, idx = (full((G + 1, H * W, M), ISENT, torch.int32) for _ in range(2))
    F._chk(lib.stem_ar_encode_batch(*net["args"], buf.data_ptr(), G, H, W, M, 2, tp.data_ptr() if tp is not None else None, hp.data_ptr(),
                                    *[t.data_ptr() for t in scratch], *net["table_args"], sym.data_ptr(), idx.data_ptr(), F._stream()))
    what = f"encode_batch {name} {hw} G={G}"
    same(host(sym), _want(ref, "sym", G), what + " sym")
    same(host(idx), _want(ref, "idx", G), what + " idx")
    same(host(buf), _want(ref, "buf", G), what + " buf")


# =========================================================================================================== decoders
def _decoders(strings):
    from spatiotemporalentropymodel_amd.entropy_models import RansDecoder
    decs = []
    for s in strings:
        decs.append(RansDecoder())
        decs[-1].set_stream(s)
    return decs


def _decode_fn():
    from spatiotemporalentropymodel_amd import _lib
    return C.cast(_lib.rans().stem_rans_decoder_decode, C.c_void_p).value


def _strings(ref, G, order=None):
    _, tables = _tables()
    pick = (lambda a: a) if order is None else (lambda a: a[order])
    return [_host_string(pick(ref["sym"][g]), pick(ref["idx"][g]), tables) for g in range(G)]


DECODE_IMAGE_CASES = [(n, hw) for n, hw, _ in ar.IMAGE_CASES]


@pytest.mark.parametrize("name,hw", DECODE_IMAGE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_decode_image_vs_reference(hip, name, hw):
    """stem_ar_decode_image on the host coder's string of the reference's symbols and indexes of image 0: the reference's buf bit for
    bit (zero ring included), the string consumed; the next image of the allocation keeps its sentinel"""
    lib, F = hip
    Gn = next(c[2] for c in ar.IMAGE_CASES if c[0] == name and c[1] == hw)
    net, ref = _net(name), ar.reference(name, hw, Gn)
    _, tables = _tables()
    H, W = hw
    M, P = net["M"], 2 * net["M"]
    target, hp, tp = _device_inputs(name, hw, Gn)
    dec = _decoders(_strings(ref, 1))[0]
    buf = _padded(np.zeros_like(target[:1]))
    scratch = [full(n, NAN) for n in (P, net["n0"], net["n1"], P)]
    idx_box, sym_box = (full(M, ISENT, torch.int32, pinned=True) for _ in range(2))
    F._chk(lib.stem_ar_decode_image(*net["args"], buf.data_ptr(), H, W, M, 2, tp[0].data_ptr() if tp is not None else None, hp[0].data_ptr(),
                                    *[t.data_ptr() for t in scratch], *net["table_args"], idx_box.data_ptr(), sym_box.data_ptr(), _decode_fn(), dec._h,
                                    *tables.args(), F._stream()))
    same(host(buf), _want(ref, "buf", 1), f"decode_image {name} {hw}")
    assert _words_left(dec, tables) is False


DECODE_BATCH_CASES = [("A", (4, 6), G) for G in range(1, 9)] + [("C", (3, 7), 3), ("D", (2, 5), 3)]


@pytest.mark.parametrize("name,hw,G", DECODE_BATCH_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_decode_batch_vs_reference(hip, name, hw, G):
    """stem_ar_decode_batch: every G = 1 .. 8 is a kernel of its own (net A); nets C and D reach its second to fourth predicated
    256-column steps"""
    lib, F = hip
    Gn = max(G, 3)
    net, ref = _net(name), ar.reference(name, hw, Gn)
    _, tables = _tables()
    H, W = hw
    M, P = net["M"], 2 * net["M"]
    target, hp, tp = _device_inputs(name, hw, G)
    decs = _decoders(_strings(ref, G))
    handles = (C.c_void_p * G)(*[d._h for d in decs])
    buf = _padded(np.zeros_like(target))
    scratch = [full((G, n), NAN) for n in (P, net["n0"], net["n1"], P)]
    idx_box, sym_box = (full((G, M), ISENT, torch.int32, pinned=True) for _ in range(2))
    F._chk(lib.stem_ar_decode_batch(*net["args"], buf.data_ptr(), G, H, W, M, 2, tp.data_ptr() if tp is not None else None, hp.data_ptr(),
                                    *[t.data_ptr() for t in scratch], *net["table_args"], idx_box.data_ptr(), sym_box.data_ptr(), _decode_fn(),
                                    C.addressof(handles), *tables.args(), F._stream()))
    same(host(buf), _want(ref, "buf", G), f"decode_batch {name} {hw} G={G}")
    assert [_words_left(d, tables) for d in decs] == [False] * G


@pytest.mark.parametrize("name,hw", [("A", (4, 6)), ("A", (3, 16)), ("B", (7, 5)), ("B", (1, 1)), ("C", (3, 7)), ("D", (2, 5))], ids=str)
def test_decode_wave_batch_vs_reference(hip, name, hw):
    """stem_ar_decode_wave_batch, G = 3, on the host coder's strings of the reference's symbols in wavefront order"""
    from spatiotemporalentropymodel_amd.codec import wave_order
    lib, F = hip
    G = 3
    net, ref = _net(name), ar.reference(name, hw, G)
    _, tables = _tables()
    H, W = hw
    M, P = net["M"], 2 * net["M"]
    target, hp, tp = _device_inputs(name, hw, G)
    decs = _decoders(_strings(ref, G, wave_order(H, W)[0]))
    handles = (C.c_void_p * G)(*[d._h for d in decs])
    npmax = min(H, (W + 2) // 3)
    buf = _padded(np.zeros_like(target))
    scratch = [full((G, npmax, n), NAN) for n in (P, net["n0"], net["n1"], P)]
    idx_box, sym_box = (full((G, npmax, M), ISENT, torch.int32, pinned=True) for _ in range(2))
    F._chk(lib.stem_ar_decode_wave_batch(*net["args"], buf.data_ptr(), G, H, W, M, 2, tp.data_ptr() if tp is not None else None, hp.data_ptr(),
                                         *[t.data_ptr() for t in scratch], *net["table_args"], idx_box.data_ptr(), sym_box.data_ptr(), _decode_fn(),
                                         C.addressof(handles), *tables.args(), F._stream()))
    same(host(buf), _want(ref, "buf", G), f"decode_wave_batch {name} {hw}")
    assert [_words_left(d, tables) for d in decs] == [False] * G


def test_persistent_decoder_supports_the_nets_it_should(hip):
    lib, _ = hip
    for name, (M, n0, n1, _tp) in ar.NETS.items():
        assert lib.stem_ar_decode_image_persistent_supported(M, n0, n1) == ar.PERSISTENT_SUPPORTED[name], name


@pytest.mark.parametrize("name,hw", [("A", (4, 6)), ("B", (4, 6)), ("C", (3, 7)), ("Dp", (2, 5))], ids=str)
def test_decode_image_persistent_vs_reference(hip, name, hw):
    """stem_ar_decode_image_persistent, called as codec._Decode.persistent_call calls it (the library keeps its own mailboxes), on the
    string of the reference's symbols: the reference's buf bit for bit -- its partial sums, continued once the symbols arrive, are the
    canonical product.  A decoder that gives up fails the test with the library's message; it is not tried again."""
    lib, F = hip
    net, ref = _net(name), ar.reference(name, hw, 1)
    _, tables = _tables()
    H, W = hw
    M, P = net["M"], 2 * net["M"]
    assert lib.stem_ar_decode_image_persistent_supported(M, net["n0"], net["n1"]) == 1
    target, hp, tp = _device_inputs(name, hw, 1)
    dec = _decoders(_strings(ref, 1))[0]
    buf = _padded(np.zeros_like(target))
    scratch = [full(n, NAN) for n in (P, net["n0"], net["n1"], P)]
    torch.cuda.synchronize()
    rc = lib.stem_ar_decode_image_persistent(*net["args"], buf.data_ptr(), H, W, M, 2, tp[0].data_ptr() if tp is not None else None, hp[0].data_ptr(),
                                             *[t.data_ptr() for t in scratch], *net["table_args"], _decode_fn(), dec._h, *tables.args(), F._stream())
    if rc != 0:
        pytest.fail(f"stem_ar_decode_image_persistent gave up ({rc}): {_last_error(lib)}")
    same(host(buf), _want(ref, "buf", 1), f"decode_image_persistent {name} {hw}")
    assert _words_left(dec, tables) is False


# =========================================================================================================== refusals
def test_gemv3_refuses_what_it_documents(hip):
    """stem_gemv3 / stem_gemv3_decode: a segment length that is no multiple of 4, a misaligned segment base, a misaligned weight, a
    write-back whose left neighbour is not the second half of a 2M segment, a table without an index mailbox: non-zero, the entry
    point named in stem_last_error, the output untouched"""
    lib, F = hip
    st = F._stream()
    N, n, M = 8, 16, 8
    W, x, x2 = full((N, 2 * n + 8), 0.5), full(n + 4, 1.0), full(2 * M, 1.0)
    sym = full(M, 1, torch.int32, pinned=True)
    mean, pix, table = full(M, 0.0), full(M, SENT), D(np.asarray(ar.TABLE, np.float32))
    y = full(N, SENT)
    ok3 = (x.data_ptr(), n, 0, None, 0, 0, None, 0, 0)
    bad_segs = {"length": (x.data_ptr(), n - 2, 0, None, 0, 0, None, 0, 0), "base": (x.data_ptr() + 4, n, 0, None, 0, 0, None, 0, 0),
                "offset": (x.data_ptr(), n, 2, None, 0, 0, None, 0, 0)}
    for what, segs in bad_segs.items():
        assert lib.stem_gemv3(W.data_ptr(), 2 * n + 8, None, *segs, y.data_ptr(), N, 0, 0.0, st) != 0, what
        assert "stem_gemv3:" in _last_error(lib), _last_error(lib)
        assert lib.stem_gemv3_decode(W.data_ptr(), 2 * n + 8, None, *segs, y.data_ptr(), N, 0, 0.0, None, None, None, M, 0, None, 0, 0.0, None, st) != 0, what
        assert "stem_gemv3_decode:" in _last_error(lib), _last_error(lib)
    for w_ptr, ldw in ((W.data_ptr() + 4, 2 * n + 8), (W.data_ptr(), 2 * n + 6)):
        assert lib.stem_gemv3(w_ptr, ldw, None, *ok3, y.data_ptr(), N, 0, 0.0, st) != 0
        assert "stem_gemv3:" in _last_error(lib)
        assert lib.stem_gemv3_decode(w_ptr, ldw, None, *ok3, y.data_ptr(), N, 0, 0.0, None, None, None, M, 0, None, 0, 0.0, None, st) != 0
        assert "stem_gemv3_decode:" in _last_error(lib)
    # prev_is_left with len2 != 2M
    segs = (x.data_ptr(), n, 0, None, 0, 0, x2.data_ptr(), 2 * M - 4, n)
    assert lib.stem_gemv3_decode(W.data_ptr(), 2 * n + 8, None, *segs, y.data_ptr(), N, 0, 0.0, sym.data_ptr(), mean.data_ptr(), pix.data_ptr(), M, 1,
                                 None, 0, 0.0, None, st) != 0
    assert "stem_gemv3_decode:" in _last_error(lib) and "write-back" in _last_error(lib)
    # a table without idx
    assert lib.stem_gemv3_decode(W.data_ptr(), 2 * n + 8, None, *ok3, y.data_ptr(), N, 0, 0.0, None, None, None, M, 0, table.data_ptr(), len(ar.TABLE),
                                 ar.BOUND, None, st) != 0
    assert "stem_gemv3_decode:" in _last_error(lib) and "index" in _last_error(lib)
    assert (host(y) == np.float32(SENT)).all() and (host(pix) == np.float32(SENT)).all()
    # and the same call with nothing wrong goes through
    F._chk(lib.stem_gemv3(W.data_ptr(), 2 * n + 8, None, *ok3, y.data_ptr(), N, 0, 0.0, st))
    same(host(y), np.full(N, 8.0, np.float32), "the accepted call")


def test_gemv3_wave_refuses_what_gemv3_refuses(hip):
    """stem_gemv3_wave loads 16 bytes at a time like stem_gemv3: a misaligned weight or segment base, a length, weight offset or stride
    that is no multiple of 4 floats, a null y, a grid without positions: non-zero, named in stem_last_error, y untouched"""
    from spatiotemporalentropymodel_amd._lib import WaveSeg as S
    lib, F = hip
    st = F._stream()
    N, n, H, Wg, t = 8, 16, 1, 1, 0
    W, x = full((N, n + 8), 0.5), full(n + 8, 1.0)
    y = full(N, SENT)

    def call(w_ptr, seg, y_ptr=None, ldw=n + 8):
        segs = (S * 3)(seg, S(None, 0, 0, 0, 0, 0), S(None, 0, 0, 0, 0, 0))
        return lib.stem_gemv3_wave(w_ptr, ldw, None, C.addressof(segs), y.data_ptr() if y_ptr is None else y_ptr, N, N, 0, 0.0, t, H, Wg, st)

    good = S(x.data_ptr(), n, 0, 0, 0, 0)
    bad = {"weight base": (W.data_ptr() + 4, good), "segment base": (W.data_ptr(), S(x.data_ptr() + 4, n, 0, 0, 0, 0)),
           "length": (W.data_ptr(), S(x.data_ptr(), n - 2, 0, 0, 0, 0)), "offset": (W.data_ptr(), S(x.data_ptr(), n, 2, 0, 0, 0)),
           "row stride": (W.data_ptr(), S(x.data_ptr(), n, 0, 2, 0, 0)), "column stride": (W.data_ptr(), S(x.data_ptr(), n, 0, 0, 2, 0)),
           "position stride": (W.data_ptr(), S(x.data_ptr(), n, 0, 0, 0, 2))}
    for what, (w_ptr, seg) in bad.items():
        assert call(w_ptr, seg) != 0, what
        assert "stem_gemv3_wave:" in _last_error(lib), _last_error(lib)
    assert call(W.data_ptr(), good, ldw=n + 6) != 0 and "stem_gemv3_wave:" in _last_error(lib)
    assert lib.stem_gemv3_wave(W.data_ptr(), n + 8, None, C.addressof((S * 3)(good, S(None, 0, 0, 0, 0, 0), S(None, 0, 0, 0, 0, 0))), None, N, N, 0, 0.0,
                               t, H, Wg, st) != 0 and "stem_gemv3_wave:" in _last_error(lib)
    segs_ok = (S * 3)(good, S(None, 0, 0, 0, 0, 0), S(None, 0, 0, 0, 0, 0))
    for Hb, Wb in ((0, 1), (1, 0)):
        assert lib.stem_gemv3_wave(W.data_ptr(), n + 8, None, C.addressof(segs_ok), y.data_ptr(), N, N, 0, 0.0, t, Hb, Wb, st) != 0
        assert "stem_gemv3_wave:" in _last_error(lib)
    assert (host(y) == np.float32(SENT)).all()
    assert call(W.data_ptr(), good) == 0
    same(host(y), np.full(N, 8.0, np.float32), "the accepted call")
