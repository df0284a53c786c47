"""An independent statement of the raster-order coding loop (csrc/ar.hip, csrc/ar_persistent.hip), numpy only.

The loop's products are specified to the bit (include/stem_ar_batch.h, "canonical product"): a mean that differs by an ulp moves
y_hat and every later context, a scale on the other side of a table entry corrupts the stream.  This module emulates that order in
float32 -- every numpy float32 operation is one IEEE rounding, as every product and sum of the kernels (compiled without FMA
contraction) is -- and states the same operations in float64.  tests/test_ar_ref.py pins it on the CPU against float64 and at
constructed ties; tests/test_hip_ar_ops.py compares every HIP form of the product, of the scale-to-index search and of the
quantisation with it bit for bit.

  gemv3 / gemv3_f64      the canonical float32 product of up to three segments; the same sum in float64 with its magnitude
  pack_ctx               masked 5x5 weight [2M, M, 5, 5] -> [2M, 12, M], the 12 live taps of the type-A mask
  wave_range             rows of wavefront step t
  index                  scale -> table index
  finish_encode / finish_decode
  encode_image           the encoder's loop in RASTER order, position by position (the kernels run it in wavefront steps)
  gp_f64_forced          the entropy parameters of every position in float64, read off a finished buffer, context by einsum
  net / case_inputs / reference / NETS / IMAGE_CASES: the nets and cases both test files iterate over

The float32 emulation assumes ordinary values: no NaN, infinity or denormal in any product, |q| < 2^23."""
import functools

import numpy as np

TABLE = (0.11, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)          # as tests/test_hip_wave_order.py
BOUND = 0.11
SLOPE = 0.01
ACT_NONE, ACT_LRELU = 0, 1
f32 = np.float32

# name -> (M, n0, n1, temporal prior)
#   A, B  the widths of tests/test_hip_wave_order.py: every segment is one partial 256-column step
#   C     5M = 260: the second step of a context row is live for lane 0 only, n0 = 264 for lanes 0-1; 2M = 104 rows are no multiple of
#         16: the last workgroup of the batched product has idle wavefronts
#   D     5M = 520; n0 = 772 is four steps, the fourth live for lane 0 only (MAXS = 4 of the lockstep decoder)
#   Dp    D with n0 = 768: the widest net the persistent decoder holds
NETS = {"A": (8, 16, 12, True), "B": (4, 16, 12, False), "C": (52, 264, 260, True), "D": (104, 772, 516, True), "Dp": (104, 768, 516, True)}
PERSISTENT_SUPPORTED = {"A": 1, "B": 1, "C": 1, "D": 0, "Dp": 1}
GEOMETRIES = ((1, 1), (1, 7), (5, 1), (4, 6), (7, 5), (3, 16))
# (net, (H, W), number of images drawn): what the whole-image encoders are compared on
IMAGE_CASES = tuple([(n, hw, 3) for n in ("A", "B") for hw in GEOMETRIES] + [("C", (3, 7), 3), ("D", (2, 5), 3), ("A", (12, 36), 9)])
WAVE_GEOMETRIES = GEOMETRIES + ((12, 36),)
# segment lengths of the single products: one step; a step and one lane | a short one; an empty first segment, two steps and one lane,
# one lane; three segments (a context window of M = 52 cut short); four full steps
SEGMENT_SETS = ((96,), (260, 8), (0, 516, 4), (8, 104, 104), (1024,))
PRODUCT_ROWS = (1, 3, 4, 6, 38)


# ------------------------------------------------------------------------------------------------------------------- the product
def _chunk_sum(p):
    """the four products of a lane's 16-byte step, added left to right"""
    return ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]


def _lane_reduce(acc):
    """64 lane accumulators [..., 64] -> lane 0 of the xor butterfly acc += acc[lane ^ off], off = 32, 16, 8, 4, 2, 1"""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ off]
    return acc[..., 0]


def _segments(W, segs, dtype):
    """-> [(x [B, len], weight columns [N, len])], B = 1 for a single input vector"""
    out = []
    for x, woff in segs:
        x = np.asarray(x, dtype)
        x = x.reshape(-1, x.shape[-1]) if x.size else np.zeros((1, 0), dtype)
        assert x.shape[-1] % 4 == 0 and woff % 4 == 0 and woff + x.shape[-1] <= W.shape[1]
        out.append((x, W[:, woff:woff + x.shape[-1]]))
    return out


def gemv3(W, bias, segs, act=ACT_NONE, slope=0.0):
    """y[n] = act(bias[n] + sum over the segments (x, woff) of W[n, woff + k] * x[k]) in the canonical float32 order.
    W [N, ldw]; x [len] -> y [N], or x [B, len] (B independent inputs, the same in every segment) -> y [B, N]."""
    W = np.asarray(W)
    assert W.dtype == f32 and len(segs) <= 3
    batched = any(np.ndim(x) == 2 for x, _ in segs)
    parts = _segments(W, segs, f32)
    B, N = max(x.shape[0] for x, _ in parts), W.shape[0]
    acc = np.zeros((B, N, 64), f32)
    for x, w in parts:
        n = x.shape[-1]
        for k0 in range(0, n, 256):
            nl = min(64, (n - k0) // 4)                                           # lanes with 4 * lane + k0 < len
            p = w[None, :, k0:k0 + 4 * nl].reshape(1, N, nl, 4) * x[:, None, k0:k0 + 4 * nl].reshape(-1, 1, nl, 4)
            acc[:, :, :nl] = acc[:, :, :nl] + _chunk_sum(p)
    v = _lane_reduce(acc)
    if bias is not None:
        v = v + np.asarray(bias, f32)
    if act == ACT_LRELU:
        v = np.where(v > 0, v, v * f32(slope))
    assert v.dtype == f32
    return v if batched else v[0]


def gemv3_depth(segs):
    """roundings on the longest path from a product to the result of gemv3 without activation: per 256-column step the product, three
    additions and the addition to the accumulator; six butterfly additions; the bias"""
    steps = sum(-(-np.shape(x)[-1] // 256) for x, _ in segs)
    return 5 * steps + 6 + 1


def gemv3_f64(W, bias, segs, act=ACT_NONE, slope=0.0):
    """-> (the same product in float64, the per-row magnitude sum |x w| + |bias| before the activation)"""
    W = np.asarray(W, np.float64)
    batched = any(np.ndim(x) == 2 for x, _ in segs)
    parts = _segments(W, segs, np.float64)
    v = sum(x @ w.T for x, w in parts)
    mag = sum(np.abs(x) @ np.abs(w).T for x, w in parts)
    if bias is not None:
        v, mag = v + np.asarray(bias, np.float64), mag + np.abs(np.asarray(bias, np.float64))
    if act == ACT_LRELU:
        v = np.where(v > 0, v, v * float(f32(slope)))
    return (v, mag) if batched else (v[0], mag[0])


# ------------------------------------------------------------------------------------------------------------------- small pieces
def pack_ctx(w):
    """[K, C, 5, 5] -> [K, 12, C]: the first 12 taps in raster order (rows 0 and 1, row 2 columns 0 and 1)"""
    w = np.asarray(w)
    K, C = w.shape[:2]
    assert w.shape[2:] == (5, 5)
    return np.ascontiguousarray(w.reshape(K, C, 25)[:, :, :12].transpose(0, 2, 1))


MASK_A = np.zeros((5, 5))
MASK_A.reshape(-1)[:12] = 1.0


def wave_range(t, H, W):
    """-> (h0, np): step t holds the positions (h, t - 3h), h = h0 .. h0 + np - 1 (np <= 0: none)"""
    lo = t - (W - 1)
    lo = (lo + 2) // 3 if lo > 0 else 0
    hi = min(t // 3, H - 1)
    return lo, hi - lo + 1


def index(scale, table, bound=BOUND):
    """T - 1 - #{t < T - 1 : max(scale, bound) <= table[t]} in float32, by entropy_ref.build_indexes (which bounds at 0.11 itself)"""
    import entropy_ref
    assert f32(bound) >= f32(entropy_ref.SCALE_BOUND)
    s = np.maximum(np.asarray(scale, f32), f32(bound))
    return entropy_ref.build_indexes(s, np.asarray(table, f32))


def index_direct(scale, table, bound=BOUND):
    """the same by the definition, in the scale's own precision against the float32 table entries (float64 scales: gp_f64_forced)"""
    scale = np.asarray(scale)
    table = np.asarray(table, f32).astype(scale.dtype)
    s = np.maximum(scale, scale.dtype.type(f32(bound)))
    return (len(table) - 1 - (s[..., None] <= table[:-1]).sum(-1)).astype(np.int32)


def finish_encode(gp, pix, table, bound=BOUND):
    """gp [..., 2M] = scales | means, pix [..., M] -> (sym int32, idx int32, pix' = q + mu) with q = rint(pix - mu), ties to even"""
    gp, pix = np.asarray(gp), np.asarray(pix)
    assert gp.dtype == f32 and pix.dtype == f32
    M = pix.shape[-1]
    mu = gp[..., M:]
    q = np.rint(pix - mu)
    return q.astype(np.int32), index(gp[..., :M], table, bound), q + mu


def finish_decode(gp, sym):
    """pix = float(sym) + mu"""
    gp, sym = np.asarray(gp), np.asarray(sym)
    assert gp.dtype == f32 and sym.dtype == np.int32
    return sym.astype(f32) + gp[..., sym.shape[-1]:]


# ------------------------------------------------------------------------------------------------------------------- the loop
def position_gp(net, buf, h, w, hp, tp):
    """the four products of position (h, w): buf [G, H+4, W+4, M] (zero ring, rows above and pixels to the left coded), hp / tp
    [G, 2M] of this position -> (ctx, h1, h2, gp), [G, .] each"""
    M = net["M"]
    G = buf.shape[0]
    P = 2 * M
    win = [(buf[:, h, w:w + 5].reshape(G, 5 * M), 0), (buf[:, h + 1, w:w + 5].reshape(G, 5 * M), 5 * M), (buf[:, h + 2, w:w + 2].reshape(G, P), 10 * M)]
    ctx = gemv3(net["w_ctx"], net["b_ctx"], win)
    pri = [(hp, 0), (ctx, P)] if tp is None else [(tp, 0), (hp, P), (ctx, 2 * P)]
    h1 = gemv3(net["w0"], net["b0"], pri, ACT_LRELU, SLOPE)
    h2 = gemv3(net["w1"], net["b1"], [(h1, 0)], ACT_LRELU, SLOPE)
    return ctx, h1, h2, gemv3(net["w2"], net["b2"], [(h2, 0)])


def encode_images(net, target, hp, tp, table=TABLE, bound=BOUND):
    """G independent images side by side (the arithmetic is per image): target [G, H, W, M], hp / tp [G, H*W, 2M] (tp may be None)
    -> sym, idx [G, H*W, M], buf [G, H+4, W+4, M], gp [G, H*W, 2M]"""
    target = np.asarray(target, f32)
    G, H, W, M = target.shape
    assert M == net["M"] and (tp is not None) == net["has_tp"]
    buf = np.zeros((G, H + 4, W + 4, M), f32)
    buf[:, 2:2 + H, 2:2 + W] = target
    sym, idx = (np.zeros((G, H * W, M), np.int32) for _ in range(2))
    gp = np.zeros((G, H * W, 2 * M), f32)
    for h in range(H):
        for w in range(W):                                                        # raster order: everything above and to the left is coded
            pos = h * W + w
            gp[:, pos] = position_gp(net, buf, h, w, hp[:, pos], None if tp is None else tp[:, pos])[3]
            sym[:, pos], idx[:, pos], buf[:, h + 2, w + 2] = finish_encode(gp[:, pos], buf[:, h + 2, w + 2], table, bound)
    return sym, idx, buf, gp


def encode_image(net, target, hp, tp, table=TABLE, bound=BOUND):
    """one image: target [H, W, M], hp / tp [H*W, 2M] -> sym, idx [H*W, M], buf [H+4, W+4, M], gp [H*W, 2M]"""
    return tuple(a[0] for a in encode_images(net, np.asarray(target)[None], np.asarray(hp)[None], None if tp is None else np.asarray(tp)[None], table, bound))


def gp_f64_forced(net, buf, hp, tp):
    """float64 entropy parameters [H*W, 2M] of every position of ONE image, teacher-forced: each position reads the finished float32
    buffer [H+4, W+4, M], so positions are independent.  The context is the masked 5x5 convolution itself (the unpacked weight times
    the type-A mask over the whole window), not the packed three-segment product."""
    buf = np.asarray(buf, np.float64)
    H, W, M = buf.shape[0] - 4, buf.shape[1] - 4, buf.shape[2]
    win = np.lib.stride_tricks.sliding_window_view(buf, (5, 5), axis=(0, 1))[:H, :W]        # [H, W, M, 5, 5]
    ctx = np.einsum("hwcij,kcij->hwk", win, net["w_ctx5"].astype(np.float64) * MASK_A).reshape(H * W, 2 * M) + net["b_ctx"]
    pri = [np.asarray(p, np.float64) for p in (tp, hp) if p is not None] + [ctx]

    def lrelu(v):
        return np.where(v > 0, v, v * float(f32(SLOPE)))

    h1 = lrelu(np.concatenate(pri, axis=1) @ net["w0"].astype(np.float64).T + net["b0"])
    h2 = lrelu(h1 @ net["w1"].astype(np.float64).T + net["b1"])
    return h2 @ net["w2"].astype(np.float64).T + net["b2"]


# ------------------------------------------------------------------------------------------------------------------- nets and cases
def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def net(name):
    """random weights of the four products, drawn as _net_host of tests/test_hip_wave_order.py draws them: the last layer's biases put
    the first channel's scale below the bound and spread the others over the table; the means stay small against the targets.
    w_ctx5 is the unpacked [2M, M, 5, 5] weight with values in its masked taps too; w_ctx [2M, 12M] is its pack."""
    M, n0, n1, has_tp = NETS[name]
    rng = np.random.default_rng(100 + sorted(NETS).index(name))
    P = 2 * M
    k0 = (3 if has_tp else 2) * P

    def rnd(*shape, scale):
        return (rng.standard_normal(shape) * scale).astype(f32)

    w2 = rnd(P, n1, scale=1.0 / n1 ** 0.5)
    w2[:M] *= f32(0.3)
    b2 = np.concatenate([np.tile(np.array([-3.0, 0.7, 3.0, 12.0], f32), M // 4), rnd(M, scale=0.5)])
    w_ctx5 = rnd(P, M, 5, 5, scale=0.6 / (12 * M) ** 0.5)
    return _frozen(dict(M=M, n0=n0, n1=n1, has_tp=has_tp, w_ctx5=w_ctx5, w_ctx=pack_ctx(w_ctx5).reshape(P, 12 * M), b_ctx=rnd(P, scale=0.2),
                        w0=rnd(n0, k0, scale=1.0 / k0 ** 0.5), b0=rnd(n0, scale=0.2), w1=rnd(n1, n0, scale=1.5 / n0 ** 0.5), b1=rnd(n1, scale=0.2),
                        w2=w2, b2=b2, table=np.array(TABLE, f32)))


@functools.lru_cache(maxsize=None)
def case_inputs(name, hw, G):
    """(target [G, H, W, M], hp [G, H*W, 2M], tp or None), drawn as _case_inputs of tests/test_hip_wave_order.py draws them (the first
    channel at least 4 from zero); image g is the same whatever G is"""
    H, W = hw
    M, has_tp = NETS[name][0], NETS[name][3]
    target, hp, tp = [], [], []
    for g in range(G):
        rng = np.random.default_rng([sorted(NETS).index(name), H, W, g])
        t = (rng.random((H, W, M)) * 12 - 6).astype(f32)
        t[..., 0] = np.where(t[..., 0] < 0, f32(-4.0), f32(4.0)) + t[..., 0] / f32(3)
        target.append(t)
        hp.append(rng.standard_normal((H * W, 2 * M)).astype(f32))
        tp.append(rng.standard_normal((H * W, 2 * M)).astype(f32))
    out = dict(target=np.stack(target), hp=np.stack(hp), tp=np.stack(tp) if has_tp else None)
    return tuple(_frozen(out).values())


@functools.lru_cache(maxsize=None)
def reference(name, hw, G):
    """encode_images of a case, computed once: dict(sym, idx, buf, gp), read-only"""
    sym, idx, buf, gp = encode_images(net(name), *case_inputs(name, hw, G))
    return _frozen(dict(sym=sym, idx=idx, buf=buf, gp=gp))


def product_case(lens, N, seed):
    """-> (W [N, ldw], bias [N], xs, woffs): a product over segments of `lens` floats whose weight columns leave gaps, are not in
    ascending order and end before the row does; with the bias the rows alternate in sign"""
    rng = np.random.default_rng(seed)
    order = [1, 2, 0][:len(lens)] if len(lens) == 3 else list(range(len(lens)))[::-1]
    woffs, col = [0] * len(lens), 4
    for i in order:                                                               # laid out in another order than they are summed
        woffs[i] = col
        col += lens[i] + 8
    ldw = col + 12
    W = (rng.standard_normal((N, ldw)) / max(sum(lens), 1) ** 0.5).astype(f32)
    xs = [rng.standard_normal(n).astype(f32) for n in lens]
    # the bias takes each row to half its dot product's magnitude, signs alternating: rows of both signs, and a result no larger than
    # the sum, so that the sum's last bits are not rounded away by the bias
    d = sum(W[:, o:o + n].astype(np.float64) @ x for x, o, n in zip(xs, woffs, lens))
    bias = (np.where(np.arange(N) % 2 == 0, 0.5, -0.5) * np.abs(d) - d).astype(f32)
    return W, bias, xs, woffs


# scales for the search: every entry, its neighbours, the bound and its neighbours, 0, -1, 1e9
def index_scales(table, bound=BOUND):
    t = np.asarray(table, f32)
    up, down, b = f32(np.inf), f32(-np.inf), f32(bound)
    return np.concatenate([t, np.nextafter(t, up), np.nextafter(t, down),
                           np.array([b, np.nextafter(b, up), np.nextafter(b, down), 0.0, -1.0, 1e9], f32)]).astype(f32)


INDEX_TABLES = ((0.11,), (0.11, 0.5), TABLE)                                      # T = 1, 2, 8
TIE_MU = 0.25
TIE_PIX = tuple(k + 0.75 for k in range(-4, 4)) + (0.5, 0.0)                       # pix - mu = k + 1/2 exactly, k = -4 .. 3; then +-0.25
TIE_SYM = (-4, -2, -2, 0, 0, 2, 2, 4, 0, 0)                                        # ties to even


def finish_case(M, table, n=1, start=0):
    """-> gp [n, 2M], pix [n, M], tie [n, M]: channel c of position p takes entry i = start + p * M + c of index_scales(table) and of
    TIE_PIX, cyclically; in every other block of len(index_scales) elements the mean is TIE_MU and the pixel the tie, in the blocks
    between both are random.  260 elements hold every scale, with a tie and with a random pixel, and every tie (scale and pixel
    are independent in the kernels: a scale meets the ties whose list position equals its own modulo 10); narrower calls walk `start`."""
    rng = np.random.default_rng([start, M, len(table)])
    sc = index_scales(table)
    i = start + np.arange(n * M)
    scales = sc[i % len(sc)]
    tie = (i // len(sc)) % 2 == 0                                                  # alternate blocks: ties, then random pixels
    mu = np.where(tie, f32(TIE_MU), rng.standard_normal(n * M).astype(f32))
    pix = np.where(tie, np.array(TIE_PIX, f32)[i % len(TIE_PIX)], (rng.random(n * M) * 12 - 6).astype(f32)).astype(f32)
    gp = np.concatenate([scales.reshape(n, M), mu.astype(f32).reshape(n, M)], axis=1)
    return gp, pix.reshape(n, M), tie.reshape(n, M)
