// Kernels for the autoregressive (raster-order) coding loop of the STEM models with a spatial prior
// (compressai/models/spatiotemporalpriors.py:916-961 encode, :1015-1054 decode).
//
// One spatial position is a chain of four matrix-vector products on a single pixel
//   ctx[2M]   = b_c + W_c[:, 12 live taps x M] . window        (masked 5x5 conv restricted to one output pixel)
//   h1[768]   = lrelu(b_0 + W_0 . (tp | hp | ctx))             (EPM.0, 1x1)
//   h2[576]   = lrelu(b_1 + W_1 . h1)                          (EPM.2)
//   gp[2M]    = b_2 + W_2 . h2                                 (EPM.4)  -> scales | means
// followed by index lookup, quantisation and write-back into the running latent buffer.  Each product
// is HBM/L2-bound (weights are read once per position): one wavefront per output row, 16-byte loads,
// reduction across the 64 lanes with wavefront shuffles.  The input vector is given as up to three
// contiguous segments so neither the 5x5 window nor cat(tp, hp, ctx) is ever materialised.
#include <chrono>

#include "ar_canon.h"
#include "../../include/stem_ar_batch.h"

// Encoder and decoder must produce the SAME floats for every entropy parameter (a mean that differs in the last bit
// shifts y_hat, which feeds later contexts; a scale on the other side of a table entry desynchronises the coder), and the
// encoder's wavefront kernels, the one-image decoder and the lockstep decoder are different kernels.  Their dot products
// are therefore all the CANONICAL PRODUCT that include/stem_ar_batch.h states (lane partials over columns 4 lane + 256 j, segment after
// segment, each 16-byte step summed left to right, xor-shuffle reduction, bias, activation).  Its arithmetic is written once, in
// ar_canon.h (dot4, wave_sum, finish, scale_index, quantise / dequantise, wave_range): the kernels below own their loops, loads and
// grids -- each measured into its form -- and call those leaves.  Everything is compiled without FMA contraction: products rounded, then
// added.  tests/ar_ref.py emulates that order in float32; tests/test_hip_ar_ops.py holds every form below to it bit for bit.
#pragma clang fp contract(off)

namespace {

struct Seg {
    const float *x;      // segment start
    int len;             // floats (multiple of 4)
    int woff;            // column offset of this segment inside a weight row
};

__global__ __launch_bounds__(256) void gemv3_kernel(const float *W, int ldw, const float *bias, Seg s0, Seg s1, Seg s2,
                                                    float *y, int N, int act, float slope)
{
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float *wr = W + (size_t)n * ldw;
    float acc = 0.f;
    const Seg segs[3] = {s0, s1, s2};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const Seg s = segs[q];
        for (int k = lane * 4; k < s.len; k += 256) {
            const f32x4 xv = *reinterpret_cast<const f32x4 *>(s.x + k);
            const f32x4 wv = *reinterpret_cast<const f32x4 *>(wr + s.woff + k);
            acc += dot4(xv, wv);
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) y[n] = finish(acc, bias ? bias[n] : 0.f, act, slope);
}

// Decoder variants of the product (two launches fewer per position):
//   head: the previous position's y_hat = symbol + mean is written back to the latent buffer by workgroup 0 and, when that
//         pixel is the left neighbour inside this window, every wavefront substitutes it on the fly for the (not yet
//         visible) buffer contents -- segment 2 is [pixel w-2 | pixel w-1];
//   tail: the last product also turns each scale into its CDF index (written to the pinned host mailbox).
struct DecodeExtra {
    const int32_t *sym_prev;   // null: plain product
    const float *mean_prev;    // gp + M of the previous position
    float *pix_prev;           // where its y_hat goes in the latent buffer
    int M, prev_is_left;
    const float *table;        // null: no index epilogue
    int T;
    float bound;
    int32_t *idx;
};

__global__ __launch_bounds__(256) void gemv3_decode_kernel(const float *W, int ldw, const float *bias, Seg s0, Seg s1, Seg s2,
                                                           float *y, int N, int act, float slope, DecodeExtra e)
{
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e.sym_prev && blockIdx.x == 0)
        for (int c = threadIdx.x; c < e.M; c += 256) e.pix_prev[c] = dequantise(e.sym_prev[c], e.mean_prev[c]);
    if (n >= N) return;
    const float *wr = W + (size_t)n * ldw;
    float acc = 0.f;
    const Seg segs[3] = {s0, s1, s2};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const Seg s = segs[q];
        const bool subst = q == 2 && e.sym_prev && e.prev_is_left;
        for (int k = lane * 4; k < s.len; k += 256) {
            f32x4 xv;
            if (subst && k >= e.M) {
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[j] = dequantise(e.sym_prev[k - e.M + j], e.mean_prev[k - e.M + j]);
            } else {
                xv = *reinterpret_cast<const f32x4 *>(s.x + k);
            }
            const f32x4 wv = *reinterpret_cast<const f32x4 *>(wr + s.woff + k);
            acc += dot4(xv, wv);
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        const float v = finish(acc, bias ? bias[n] : 0.f, act, slope);
        y[n] = v;
        if (e.table && n < e.M) e.idx[n] = scale_index(v, e.bound, e.table, e.T);
    }
}

// encode side: index = build_indexes(scale), symbol = round(target - mean), buffer <- symbol + mean
__global__ void ar_finish_encode_kernel(const float *gp, const float *table, int T, float scale_bound, float *pix,
                                        int32_t *sym, int32_t *idx, int M)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= M) return;
    const float mu = gp[M + c];
    const int k = scale_index(gp[c], scale_bound, table, T);
    float q;
    pix[c] = quantise(pix[c], mu, q);
    sym[c] = (int32_t)q;
    idx[c] = k;
}
__global__ void ar_index_kernel(const float *gp, const float *table, int T, float scale_bound, int32_t *idx, int M)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= M) return;
    idx[c] = scale_index(gp[c], scale_bound, table, T);
}
// decode side: buffer <- symbol + mean  (EntropyModel.dequantize, entropy_models.py:156-163)
__global__ void ar_finish_decode_kernel(const float *gp, const int32_t *sym, float *pix, int M)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= M) return;
    pix[c] = dequantise(sym[c], gp[M + c]);
}

// masked conv weight [2M][M][5][5] -> [2M][12 live taps][M]  (live taps of the type-A mask: rows 0,1 full, row 2 cols 0,1)
__global__ void pack_ctx_gemv_kernel(const float *w, float *out, int K, int C)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)K * 12 * C) return;
    const int c = (int)(i % C);
    const int t = (int)((i / C) % 12);
    const int k = (int)(i / ((size_t)12 * C));
    out[i] = w[((size_t)k * C + c) * 25 + t];      // live taps are exactly the first 12 of the 25 in raster order
}

int seg_ok(const Seg &s) { return s.len == 0 || (s.x && (s.len % 4 == 0) && (s.woff % 4 == 0) && (((uintptr_t)s.x & 15) == 0)); }

}   // namespace

STEM_EXPORT int stem_gemv3(const float *W, int ldw, const float *bias, const float *x0, int len0, int woff0,
                           const float *x1, int len1, int woff1, const float *x2, int len2, int woff2, float *y, int N,
                           int act, float slope, void *stream)
{
    STEM_CHECK_ARG(W && y && N > 0 && ldw % 4 == 0 && (((uintptr_t)W & 15) == 0), "stem_gemv3: bad arguments");
    Seg s0{x0, len0, woff0}, s1{x1, len1, woff1}, s2{x2, len2, woff2};
    STEM_CHECK_ARG(seg_ok(s0) && seg_ok(s1) && seg_ok(s2), "stem_gemv3: segments must be 16-byte aligned multiples of 4 floats");
    hipLaunchKernelGGL(gemv3_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, W, ldw, bias, s0, s1, s2, y, N, act, slope);
    STEM_LAUNCH_CHECK("gemv3");
    return 0;
}

STEM_EXPORT int stem_gemv3_decode(const float *W, int ldw, const float *bias, const float *x0, int len0, int woff0,
                                  const float *x1, int len1, int woff1, const float *x2, int len2, int woff2, float *y, int N,
                                  int act, float slope, const int32_t *sym_prev, const float *mean_prev, float *pix_prev, int M,
                                  int prev_is_left, const float *table, int T, float scale_bound, int32_t *idx, void *stream)
{
    STEM_CHECK_ARG(W && y && N > 0 && ldw % 4 == 0 && (((uintptr_t)W & 15) == 0) && M % 4 == 0, "stem_gemv3_decode: bad arguments");
    Seg s0{x0, len0, woff0}, s1{x1, len1, woff1}, s2{x2, len2, woff2};
    STEM_CHECK_ARG(seg_ok(s0) && seg_ok(s1) && seg_ok(s2), "stem_gemv3_decode: segments must be 16-byte aligned multiples of 4 floats");
    STEM_CHECK_ARG(!sym_prev || (mean_prev && pix_prev && (!prev_is_left || len2 == 2 * M)), "stem_gemv3_decode: inconsistent write-back arguments");
    STEM_CHECK_ARG(!table || (idx && T >= 1 && M <= N), "stem_gemv3_decode: inconsistent index arguments");
    DecodeExtra e{sym_prev, mean_prev, pix_prev, M, prev_is_left, table, T, scale_bound, idx};
    hipLaunchKernelGGL(gemv3_decode_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, W, ldw, bias, s0, s1, s2, y, N, act, slope, e);
    STEM_LAUNCH_CHECK("gemv3_decode");
    return 0;
}

STEM_EXPORT int stem_pack_ctx_gemv(const float *w, float *out, int K, int C, void *stream)
{
    STEM_CHECK_ARG(w && out && K > 0 && C > 0, "stem_pack_ctx_gemv: bad arguments");
    const size_t n = (size_t)K * 12 * C;
    hipLaunchKernelGGL(pack_ctx_gemv_kernel, dim3((unsigned)cdivz(n, 256)), dim3(256), 0, (hipStream_t)stream, w, out, K, C);
    STEM_LAUNCH_CHECK("pack_ctx_gemv");
    return 0;
}

STEM_EXPORT int stem_ar_finish_encode(const float *gp, const float *table, int T, float scale_bound, float *pix,
                                      int32_t *sym, int32_t *idx, int M, void *stream)
{
    STEM_CHECK_ARG(gp && table && pix && sym && idx && M > 0 && T >= 1, "stem_ar_finish_encode: bad arguments");
    hipLaunchKernelGGL(ar_finish_encode_kernel, dim3(cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream, gp, table, T, scale_bound,
                       pix, sym, idx, M);
    STEM_LAUNCH_CHECK("ar_finish_encode");
    return 0;
}

STEM_EXPORT int stem_ar_index(const float *gp, const float *table, int T, float scale_bound, int32_t *idx, int M, void *stream)
{
    STEM_CHECK_ARG(gp && table && idx && M > 0 && T >= 1, "stem_ar_index: bad arguments");
    hipLaunchKernelGGL(ar_index_kernel, dim3(cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream, gp, table, T, scale_bound, idx, M);
    STEM_LAUNCH_CHECK("ar_index");
    return 0;
}

STEM_EXPORT int stem_ar_finish_decode(const float *gp, const int32_t *sym, float *pix, int M, void *stream)
{
    STEM_CHECK_ARG(gp && sym && pix && M > 0, "stem_ar_finish_decode: bad arguments");
    hipLaunchKernelGGL(ar_finish_decode_kernel, dim3(cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream, gp, sym, pix, M);
    STEM_LAUNCH_CHECK("ar_finish_decode");
    return 0;
}

// ================================================================================================
// Wavefront-parallel ENCODER.  With a 5x5 type-A mask and raster order, position (h, w) depends on
// (h, w-1..w-2) and on rows h-1, h-2 at columns w-2..w+2, so all positions with the same t = w + 3h are
// mutually independent: a frame of H x W latents needs W + 3(H-1) steps (321 for 68 x 120) instead of H*W
// (8160), each step a *batch* of up to min(H, W/3) pixels.  Symbols and indexes land in raster order, so the
// host coder produces the same bytes as the sequential loop.  (The decoder cannot do this: the rANS stream
// itself is sequential in raster order.)
//
// Batched matrix-vector product: one wavefront per output row n, looping over the step's positions so the
// weight row stays in L1; the input of position p is up to three segments at offsets sh*h + sw*w + sp*p.
namespace {

struct WSeg {
    const float *x;
    int len, woff;
    long sh, sw, sp;
};

constexpr int WAVE_ROWS = 24;     // workgroup rows over which the positions of one wavefront step are spread (more waves in flight)

__global__ __launch_bounds__(256) void gemv3_wave_kernel(const float *W, int ldw, const float *bias, WSeg s0, WSeg s1, WSeg s2,
                                                         float *y, int ldy, int N, int act, float slope, int t, int H, int Wd)
{
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    int h0, np;
    wave_range(t, H, Wd, h0, np);
    const float *wr = W + (size_t)n * ldw;
    const float b = bias ? bias[n] : 0.f;
    const WSeg segs[3] = {s0, s1, s2};
    for (int p = blockIdx.y; p < np; p += gridDim.y) {      // positions of the step are spread over gridDim.y workgroup rows
        const int h = h0 + p, w = t - 3 * h;
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const WSeg s = segs[q];
            const float *xp = s.x + s.sh * h + s.sw * w + s.sp * p;
            for (int k = lane * 4; k < s.len; k += 256) {
                const f32x4 xv = *reinterpret_cast<const f32x4 *>(xp + k);
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(wr + s.woff + k);
                acc += dot4(xv, wv);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) y[(size_t)p * ldy + n] = finish(acc, b, act, slope);
    }
}

__global__ void ar_finish_encode_wave_kernel(const float *gp, const float *table, int T, float scale_bound, float *buf,
                                             int32_t *sym, int32_t *idx, int M, int t, int H, int Wd, int Wp, int pad)
{
    int h0, np;
    wave_range(t, H, Wd, h0, np);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np * M) return;
    const int p = i / M, c = i - p * M;
    const int h = h0 + p, w = t - 3 * h;
    const float *g = gp + (size_t)p * 2 * M;
    const float mu = g[M + c];
    const int k = scale_index(g[c], scale_bound, table, T);
    float *pix = buf + ((size_t)(h + pad) * Wp + (w + pad)) * M;
    float q;
    pix[c] = quantise(pix[c], mu, q);
    const size_t o = ((size_t)h * Wd + w) * M + c;
    sym[o] = (int32_t)q;
    idx[o] = k;
}

}   // namespace

STEM_EXPORT int stem_gemv3_wave(const float *W, int ldw, const float *bias, const stem_wave_seg *segs, float *y, int ldy, int N,
                                int act, float slope, int t, int H, int Wd, void *stream)
{
    // the kernel loads 16 bytes at a time from W + n * ldw + woff + k and from x + sh * h + sw * w + sp * p + k: what stem_gemv3 asks of
    // its weight and segments, plus strides that keep every position's segment aligned
    STEM_CHECK_ARG(W && segs && y && N > 0 && H > 0 && Wd > 0 && ldw % 4 == 0 && (((uintptr_t)W & 15) == 0), "stem_gemv3_wave: bad arguments");
    WSeg s[3];
    for (int i = 0; i < 3; ++i) {
        s[i].x = segs[i].x; s[i].len = segs[i].len; s[i].woff = segs[i].woff;
        s[i].sh = segs[i].sh; s[i].sw = segs[i].sw; s[i].sp = segs[i].sp;
        STEM_CHECK_ARG(s[i].len == 0 || (s[i].x && (((uintptr_t)s[i].x & 15) == 0) && s[i].len % 4 == 0 && s[i].woff % 4 == 0 && s[i].sh % 4 == 0 &&
                                         s[i].sw % 4 == 0 && s[i].sp % 4 == 0),
                       "stem_gemv3_wave: segment %d is not a 16-byte aligned multiple of 4 floats with strides of multiples of 4 floats", i);
    }
    const int maxp = H < (Wd + 2) / 3 ? H : (Wd + 2) / 3;
    hipLaunchKernelGGL(gemv3_wave_kernel, dim3(cdiv(N, 4), maxp < WAVE_ROWS ? maxp : WAVE_ROWS), dim3(256), 0, (hipStream_t)stream, W, ldw, bias,
                       s[0], s[1], s[2], y, ldy, N, act, slope, t, H, Wd);
    STEM_LAUNCH_CHECK("gemv3_wave");
    return 0;
}

STEM_EXPORT int stem_ar_finish_encode_wave(const float *gp, const float *table, int T, float scale_bound, float *buf,
                                           int32_t *sym, int32_t *idx, int M, int t, int H, int Wd, int Wp, int pad, void *stream)
{
    STEM_CHECK_ARG(gp && table && buf && sym && idx && M > 0 && T >= 1, "stem_ar_finish_encode_wave: bad arguments");
    const int maxp = H < (Wd + 2) / 3 ? H : (Wd + 2) / 3;
    hipLaunchKernelGGL(ar_finish_encode_wave_kernel, dim3(cdiv(maxp * M, 256)), dim3(256), 0, (hipStream_t)stream, gp, table, T,
                       scale_bound, buf, sym, idx, M, t, H, Wd, Wp, pad);
    STEM_LAUNCH_CHECK("ar_finish_encode_wave");
    return 0;
}

// ================================================================================================
// DECODER, whole image: the raster-order loop of spatiotemporalpriors.py:1015-1054 as ONE C-ABI call.  Per position: four
// launches (context + write-back of the previous pixel, EPM.0, EPM.2, EPM.4 + CDF indexes), one stream synchronisation,
// and one call of the host symbol decoder (a C function pointer -- stem_rans_decoder_decode of libstem_rans -- so the two
// libraries stay independent) through the pinned mailbox.  No interpreter in the loop: ~30 us per position instead of ~45.
STEM_EXPORT int stem_ar_decode_image(const float *w_ctx, int ld_ctx, const float *b_ctx, const float *w0, int ld0, const float *b0, int n0,
                                     const float *w1, int ld1, const float *b1, int n1, const float *w2, int ld2, const float *b2,
                                     float *buf, int H, int W, int M, int pad, const float *tp, const float *hp,
                                     float *ctx, float *h1, float *h2, float *gp, const float *table, int T, float scale_bound, float slope,
                                     int32_t *idx_host, int32_t *sym_host, stem_symbol_decoder_fn decode, void *dec,
                                     const int32_t *cdfs, int ncdf, int cdf_stride, const int32_t *sizes, const int32_t *offsets, void *stream)
{
    STEM_CHECK_ARG(w_ctx && b_ctx && w0 && b0 && w1 && b1 && w2 && b2 && buf && hp && ctx && h1 && h2 && gp && table && idx_host && sym_host && decode,
                   "stem_ar_decode_image: null pointer");
    STEM_CHECK_ARG(H > 0 && W > 0 && M > 0 && M % 4 == 0 && n0 % 4 == 0 && n1 % 4 == 0 && ld_ctx % 4 == 0 && ld0 % 4 == 0 && ld1 % 4 == 0 &&
                   ld2 % 4 == 0 && T >= 1 && pad == 2, "stem_ar_decode_image: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const int P = 2 * M, Wp = W + 2 * pad;
    float *pix_prev = nullptr;
    const DecodeExtra none{nullptr, nullptr, nullptr, M, 0, nullptr, 0, 0.f, nullptr};
    for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w) {
            const size_t pos = (size_t)h * W + w;
            const float *r0 = buf + ((size_t)h * Wp + w) * M, *r1 = r0 + (size_t)Wp * M, *r2 = r1 + (size_t)Wp * M;
            DecodeExtra head = none;
            if (pix_prev && w == 0 && W <= 3) {
                // a latent of at most three columns: the previous position (h-1, W-1) lies in the rows ABOVE this window, where the
                // context product reads the buffer itself -- the write-back folded into that launch would race with those reads, so
                // the pixel is committed by a launch of its own first (same float: symbol + mean)
                hipLaunchKernelGGL(ar_finish_decode_kernel, dim3(cdiv(M, 256)), dim3(256), 0, st, gp, sym_host, pix_prev, M);
            } else if (pix_prev) {
                head.sym_prev = sym_host; head.mean_prev = gp + M; head.pix_prev = pix_prev; head.prev_is_left = w > 0 ? 1 : 0;
            }
            hipLaunchKernelGGL(gemv3_decode_kernel, dim3(cdiv(P, 4)), dim3(256), 0, st, w_ctx, ld_ctx, b_ctx, Seg{r0, 5 * M, 0}, Seg{r1, 5 * M, 5 * M},
                               Seg{r2, 2 * M, 10 * M}, ctx, P, 0, 0.f, head);
            const float *hp_pix = hp + pos * P;
            if (tp)
                hipLaunchKernelGGL(gemv3_kernel, dim3(cdiv(n0, 4)), dim3(256), 0, st, w0, ld0, b0, Seg{tp + pos * P, P, 0}, Seg{hp_pix, P, P},
                                   Seg{ctx, P, 2 * P}, h1, n0, (int)STEM_ACT_LRELU, slope);
            else
                hipLaunchKernelGGL(gemv3_kernel, dim3(cdiv(n0, 4)), dim3(256), 0, st, w0, ld0, b0, Seg{hp_pix, P, 0}, Seg{ctx, P, P},
                                   Seg{nullptr, 0, 0}, h1, n0, (int)STEM_ACT_LRELU, slope);
            hipLaunchKernelGGL(gemv3_kernel, dim3(cdiv(n1, 4)), dim3(256), 0, st, w1, ld1, b1, Seg{h1, n0, 0}, Seg{nullptr, 0, 0},
                               Seg{nullptr, 0, 0}, h2, n1, (int)STEM_ACT_LRELU, slope);
            DecodeExtra tail = none;
            tail.table = table; tail.T = T; tail.bound = scale_bound; tail.idx = idx_host;
            hipLaunchKernelGGL(gemv3_decode_kernel, dim3(cdiv(P, 4)), dim3(256), 0, st, w2, ld2, b2, Seg{h2, n1, 0}, Seg{nullptr, 0, 0},
                               Seg{nullptr, 0, 0}, gp, P, 0, 0.f, tail);
            if (hipStreamSynchronize(st) != hipSuccess) {
                stem_set_error("stem_ar_decode_image: device error at position (%d, %d): %s", h, w, hipGetErrorString(hipGetLastError()));
                return -2;
            }
            if (int rc = decode(dec, idx_host, (size_t)M, cdfs, ncdf, cdf_stride, sizes, offsets, sym_host)) {
                stem_set_error("stem_ar_decode_image: host symbol decoder failed (%d) at position (%d, %d)", rc, h, w);
                return -3;
            }
            pix_prev = buf + ((size_t)(h + pad) * Wp + (w + pad)) * M;
        }
    hipLaunchKernelGGL(ar_finish_decode_kernel, dim3(cdiv(M, 256)), dim3(256), 0, st, gp, sym_host, pix_prev, M);
    STEM_LAUNCH_CHECK("ar_decode_image");
    return 0;
}

// ENCODER, whole image: the W + 3(H-1) wavefront steps of the section above queued by one C-ABI call (5 launches per step,
// no synchronisation): the host then makes a single rANS call on the raster-ordered symbols / indexes.
STEM_EXPORT int stem_ar_encode_image(const float *w_ctx, int ld_ctx, const float *b_ctx, const float *w0, int ld0, const float *b0, int n0,
                                     const float *w1, int ld1, const float *b1, int n1, const float *w2, int ld2, const float *b2,
                                     float *buf, int H, int W, int M, int pad, const float *tp, const float *hp,
                                     float *wctx, float *wh1, float *wh2, float *wgp, const float *table, int T, float scale_bound,
                                     float slope, int32_t *sym, int32_t *idx, void *stream)
{
    STEM_CHECK_ARG(w_ctx && b_ctx && w0 && b0 && w1 && b1 && w2 && b2 && buf && hp && wctx && wh1 && wh2 && wgp && table && sym && idx,
                   "stem_ar_encode_image: null pointer");
    STEM_CHECK_ARG(H > 0 && W > 0 && M > 0 && M % 4 == 0 && n0 % 4 == 0 && n1 % 4 == 0 && pad == 2 && T >= 1, "stem_ar_encode_image: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const int P = 2 * M, Wp = W + 2 * pad;
    const long row = (long)Wp * M;
    const int maxp = H < (W + 2) / 3 ? H : (W + 2) / 3;
    const WSeg none{nullptr, 0, 0, 0, 0, 0};
    // context window of position (h, w): rows h, h+1 (5 pixels) and h+2 (2 pixels) of the padded buffer, starting at column w
    const WSeg c0{buf, 5 * M, 0, row, M, 0}, c1{buf + row, 5 * M, 5 * M, row, M, 0}, c2{buf + 2 * row, 2 * M, 10 * M, row, M, 0};
    const WSeg sctx{wctx, P, tp ? 2 * P : P, 0, 0, P};
    const WSeg stp{tp, P, 0, (long)W * P, P, 0}, shp{hp, P, tp ? P : 0, (long)W * P, P, 0};
    const WSeg sh1{wh1, n0, 0, 0, 0, n0}, sh2{wh2, n1, 0, 0, 0, n1};
    const int gy = maxp < WAVE_ROWS ? maxp : WAVE_ROWS;
    for (int t = 0; t < W + 3 * (H - 1); ++t) {
        hipLaunchKernelGGL(gemv3_wave_kernel, dim3(cdiv(P, 4), gy), dim3(256), 0, st, w_ctx, ld_ctx, b_ctx, c0, c1, c2, wctx, P, P, 0, 0.f, t, H, W);
        if (tp)
            hipLaunchKernelGGL(gemv3_wave_kernel, dim3(cdiv(n0, 4), gy), dim3(256), 0, st, w0, ld0, b0, stp, shp, sctx, wh1, n0, n0,
                               (int)STEM_ACT_LRELU, slope, t, H, W);
        else
            hipLaunchKernelGGL(gemv3_wave_kernel, dim3(cdiv(n0, 4), gy), dim3(256), 0, st, w0, ld0, b0, shp, sctx, none, wh1, n0, n0,
                               (int)STEM_ACT_LRELU, slope, t, H, W);
        hipLaunchKernelGGL(gemv3_wave_kernel, dim3(cdiv(n1, 4), gy), dim3(256), 0, st, w1, ld1, b1, sh1, none, none, wh2, n1, n1,
                           (int)STEM_ACT_LRELU, slope, t, H, W);
        hipLaunchKernelGGL(gemv3_wave_kernel, dim3(cdiv(P, 4), gy), dim3(256), 0, st, w2, ld2, b2, sh2, none, none, wgp, P, P, 0, 0.f, t, H, W);
        hipLaunchKernelGGL(ar_finish_encode_wave_kernel, dim3(cdiv(maxp * M, 256)), dim3(256), 0, st, wgp, table, T, scale_bound, buf, sym, idx,
                           M, t, H, W, Wp, pad);
    }
    STEM_LAUNCH_CHECK("ar_encode_image");
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// DECODER, G images in lockstep.  The raster-order chain (the context of a position needs the previous position's symbols,
// which needed that position's entropy parameters ...) makes ONE image latency-bound: ~35 us per position for four
// dependent dispatches + a host round trip, whatever the arithmetic costs.  Independent images (the batch elements of
// decompress(), i.e. different sequences / GOPs: spatiotemporalpriors.py:1015-1054 loops over them one after the other)
// share that latency: the same four launches advance all G images by one position -- every wavefront still owns one
// output row, loads its weight row ONCE and accumulates G dot products in the single-image order, so every image's floats
// (hence symbols, indexes and bytes) are exactly those of stem_ar_decode_image.
namespace {

constexpr int GMAX = 8;
struct SegB {
    const float *x;      // image 0
    int len, woff;
    long stride;         // floats between consecutive images
};
struct DecodeExtraB {
    const int32_t *sym_prev;   // [G][M] (pinned host), null: plain product
    const float *mean_prev;    // gp + M of image 0, image stride gp_stride
    float *pix_prev;           // image 0, image stride buf_stride
    long gp_stride, buf_stride;
    int M, prev_is_left;
    const float *table;
    int T;
    float bound;
    int32_t *idx;              // [G][M] (pinned host)
};

// One wavefront per output row (the products are latency-bound: what counts is how many independent loads are in flight,
// row-blocked variants with fewer wavefronts were 2x slower).  G is a template parameter and each segment is walked in up to
// MAXS fully unrolled 256-column steps, so that the weight loads of a segment, then each image's x loads, are issued back to
// back instead of one exposed latency per step.  Every (row, image) sum accumulates its steps in ascending k: the canonical
// product of include/stem_ar_batch.h -- the order, and therefore the bits, of gemv3_decode_kernel.
constexpr int MAXS = 4;          // segments of up to 1024 floats (5 M = 960 for M = 192, n0 = 768)
template <int G>
__global__ __launch_bounds__(256) void gemv3b_decode_kernel(const float *W, int ldw, const float *bias, SegB s0, SegB s1, SegB s2,
                                                            float *y, long ystride, int N, int act, float slope, DecodeExtraB e)
{
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float *wr = W + (size_t)n * ldw;
    float acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.f;
    const SegB segs[3] = {s0, s1, s2};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const SegB s = segs[q];
        if (s.len == 0) continue;
        f32x4 wv[MAXS];
        bool ok[MAXS];
#pragma unroll
        for (int t = 0; t < MAXS; ++t) {
            const int k = lane * 4 + 256 * t;
            ok[t] = k < s.len;
            wv[t] = *reinterpret_cast<const f32x4 *>(wr + s.woff + (ok[t] ? k : 0));
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            f32x4 xv[MAXS];
#pragma unroll
            for (int t = 0; t < MAXS; ++t) xv[t] = *reinterpret_cast<const f32x4 *>(s.x + g * s.stride + (ok[t] ? lane * 4 + 256 * t : 0));
#pragma unroll
            for (int t = 0; t < MAXS; ++t) {
                const float d = dot4(xv[t], wv[t]);
                acc[g] = ok[t] ? acc[g] + d : acc[g];
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float a = wave_sum(acc[g]);
        if (lane == 0) {
            const float v = finish(a, bias ? bias[n] : 0.f, act, slope);
            y[g * ystride + n] = v;
            if (e.table && n < e.M) e.idx[g * e.M + n] = scale_index(v, e.bound, e.table, e.T);
        }
    }
}

template <int G>
void launch_gemv3b(hipStream_t st, int N, const float *W, int ldw, const float *bias, SegB a, SegB b, SegB c, float *y, long ystride, int act,
                   float slope, const DecodeExtraB &e)
{
    hipLaunchKernelGGL((gemv3b_decode_kernel<G>), dim3(cdiv(N, 4)), dim3(256), 0, st, W, ldw, bias, a, b, c, y, ystride, N, act, slope, e);
}
void launch_gemv3b_g(int G, hipStream_t st, int N, const float *W, int ldw, const float *bias, SegB a, SegB b, SegB c, float *y, long ystride,
                     int act, float slope, const DecodeExtraB &e)
{
    switch (G) {
    case 1: launch_gemv3b<1>(st, N, W, ldw, bias, a, b, c, y, ystride, act, slope, e); break;
    case 2: launch_gemv3b<2>(st, N, W, ldw, bias, a, b, c, y, ystride, act, slope, e); break;
    case 3: launch_gemv3b<3>(st, N, W, ldw, bias, a, b, c, y, ystride, act, slope, e); break;
    case 4: launch_gemv3b<4>(st, N, W, ldw, bias, a, b, c, y, ystride, act, slope, e); break;
    case 5: launch_gemv3b<5>(st, N, W, ldw, bias, a, b, c, y, ystride, act, slope, e); break;
    case 6: launch_gemv3b<6>(st, N, W, ldw, bias, a, b, c, y, ystride, act, slope, e); break;
    case 7: launch_gemv3b<7>(st, N, W, ldw, bias, a, b, c, y, ystride, act, slope, e); break;
    default: launch_gemv3b<8>(st, N, W, ldw, bias, a, b, c, y, ystride, act, slope, e); break;
    }
}

__global__ void ar_finish_decode_batch_kernel(const float *gp, long gp_stride, const int32_t *sym, float *pix, long buf_stride, int M, int G)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * G) return;
    const int g = i / M, c = i - g * M;
    pix[g * buf_stride + c] = dequantise(sym[g * M + c], gp[g * gp_stride + M + c]);
}

// STEM_AR_PROFILE: where a decoder step's time goes -- queueing the launches, waiting for the stream, the host coder -- summed over a call
struct StepTimer {
    const bool on;
    double launch = 0, wait = 0, host = 0, mark[3] = {0, 0, 0};
    StepTimer() : on(enabled()) {}
    static bool enabled()
    {
        static const bool prof = getenv("STEM_AR_PROFILE") != nullptr;
        return prof;
    }
    static double now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void at(int i) { if (on) mark[i] = now(); }       // 0: the step begins, 1: its launches are queued, 2: the stream has drained
    void step_done()                                   // ... and the host coder has returned
    {
        if (!on) return;
        launch += mark[1] - mark[0]; wait += mark[2] - mark[1]; host += now() - mark[2];
    }
};

}   // namespace

STEM_EXPORT int stem_ar_decode_batch(const float *w_ctx, int ld_ctx, const float *b_ctx, const float *w0, int ld0, const float *b0, int n0,
                                     const float *w1, int ld1, const float *b1, int n1, const float *w2, int ld2, const float *b2,
                                     float *buf, int G, int H, int W, int M, int pad, const float *tp, const float *hp,
                                     float *ctx, float *h1, float *h2, float *gp, const float *table, int T, float scale_bound, float slope,
                                     int32_t *idx_host, int32_t *sym_host, stem_symbol_decoder_fn decode, void *const *decs,
                                     const int32_t *cdfs, int ncdf, int cdf_stride, const int32_t *sizes, const int32_t *offsets, void *stream)
{
    STEM_CHECK_ARG(w_ctx && b_ctx && w0 && b0 && w1 && b1 && w2 && b2 && buf && hp && ctx && h1 && h2 && gp && table && idx_host && sym_host && decode && decs,
                   "stem_ar_decode_batch: null pointer");
    STEM_CHECK_ARG(G >= 1 && G <= GMAX, "stem_ar_decode_batch: 1..%d images per call, got %d", GMAX, G);
    STEM_CHECK_ARG(5 * M <= 256 * MAXS && n0 <= 256 * MAXS && n1 <= 256 * MAXS, "stem_ar_decode_batch: segments longer than %d floats (M=%d n0=%d n1=%d)",
                   256 * MAXS, M, n0, n1);
    STEM_CHECK_ARG(H > 0 && W > 0 && M > 0 && M % 4 == 0 && n0 % 4 == 0 && n1 % 4 == 0 && ld_ctx % 4 == 0 && ld0 % 4 == 0 && ld1 % 4 == 0 &&
                   ld2 % 4 == 0 && T >= 1 && pad == 2, "stem_ar_decode_batch: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const int P = 2 * M, Wp = W + 2 * pad;
    const long bufs = (long)(H + 2 * pad) * Wp * M, pris = (long)H * W * P;        // image strides of buf and of tp / hp
    float *pix_prev = nullptr;
    StepTimer tm;
    DecodeExtraB none;
    memset(&none, 0, sizeof(none));
    none.M = M; none.gp_stride = P; none.buf_stride = bufs;
    const SegB nil{nullptr, 0, 0, 0};
    for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w) {
            const size_t pos = (size_t)h * W + w;
            tm.at(0);
            const float *r0 = buf + ((size_t)h * Wp + w) * M, *r1 = r0 + (size_t)Wp * M, *r2 = r1 + (size_t)Wp * M;
            // The previous position's symbols arrive in the pinned host mailbox.  The one-image loop lets every wavefront of
            // the context product substitute them on the fly (saving a launch); with G images that is 2M x G floats fetched
            // over PCIe by each of the 2M rows (measured: 90 of 110 us per step at G = 8), so here a one-workgroup kernel
            // commits y_hat = symbol + mean to the latent buffers first and the product reads device memory only.
            const DecodeExtraB head = none;
            if (pix_prev)
                hipLaunchKernelGGL(ar_finish_decode_batch_kernel, dim3(cdiv(M * G, 256)), dim3(256), 0, st, gp, (long)P, sym_host, pix_prev, bufs, M, G);
            launch_gemv3b_g(G, st, P, w_ctx, ld_ctx, b_ctx, SegB{r0, 5 * M, 0, bufs}, SegB{r1, 5 * M, 5 * M, bufs}, SegB{r2, 2 * M, 10 * M, bufs},
                            ctx, (long)P, 0, 0.f, head);
            const float *hp_pix = hp + pos * P;
            if (tp)
                launch_gemv3b_g(G, st, n0, w0, ld0, b0, SegB{tp + pos * P, P, 0, pris}, SegB{hp_pix, P, P, pris}, SegB{ctx, P, 2 * P, (long)P},
                                h1, (long)n0, (int)STEM_ACT_LRELU, slope, none);
            else
                launch_gemv3b_g(G, st, n0, w0, ld0, b0, SegB{hp_pix, P, 0, pris}, SegB{ctx, P, P, (long)P}, nil, h1, (long)n0,
                                (int)STEM_ACT_LRELU, slope, none);
            launch_gemv3b_g(G, st, n1, w1, ld1, b1, SegB{h1, n0, 0, (long)n0}, nil, nil, h2, (long)n1, (int)STEM_ACT_LRELU, slope, none);
            DecodeExtraB tail = none;
            tail.table = table; tail.T = T; tail.bound = scale_bound; tail.idx = idx_host;
            launch_gemv3b_g(G, st, P, w2, ld2, b2, SegB{h2, n1, 0, (long)n1}, nil, nil, gp, (long)P, 0, 0.f, tail);
            tm.at(1);
            if (hipStreamSynchronize(st) != hipSuccess) {
                stem_set_error("stem_ar_decode_batch: device error at position (%d, %d): %s", h, w, hipGetErrorString(hipGetLastError()));
                return -2;
            }
            tm.at(2);
            for (int g = 0; g < G; ++g)
                if (int rc = decode(decs[g], idx_host + (size_t)g * M, (size_t)M, cdfs, ncdf, cdf_stride, sizes, offsets, sym_host + (size_t)g * M)) {
                    stem_set_error("stem_ar_decode_batch: host symbol decoder failed (%d) for image %d at position (%d, %d)", rc, g, h, w);
                    return -3;
                }
            pix_prev = buf + ((size_t)(h + pad) * Wp + (w + pad)) * M;
            tm.step_done();
        }
    if (tm.on)
        fprintf(stderr, "[ar decode batch] G=%d positions=%d: launch %.1f us, wait %.1f us, host coder %.1f us per position step\n", G, H * W,
                tm.launch / (H * W), tm.wait / (H * W), tm.host / (H * W));
    hipLaunchKernelGGL(ar_finish_decode_batch_kernel, dim3(cdiv(M * G, 256)), dim3(256), 0, st, gp, (long)P, sym_host, pix_prev, bufs, M, G);
    STEM_LAUNCH_CHECK("ar_decode_batch");
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// ENCODER, G images in lockstep: the counterpart of stem_ar_decode_batch.  One image's wavefront step is five launches of a few
// microseconds of work each, so W + 3(H-1) steps cost their launch latency; G independent images (the GOP chains of
// evaluation.eval_sequence, the batch elements of compress()) share it: the same five launches cover the G * np positions of
// step t.  The image index is folded into the position loop (j = g * np + p), every wavefront still spreads each dot product over its 64 lanes, and
// a wavefront takes WAVE_R rows and up to WAVE_U positions at once: a register tile of WAVE_R * WAVE_U dot products fed by
// WAVE_R + WAVE_U loads per k step.  Every (image, position, row) sum is accumulated exactly as
// gemv3_wave_kernel does it -- k = lane * 4, += 256, segment after segment, xor-shuffle reduction: the canonical product of
// include/stem_ar_batch.h -- so each image's floats, symbols and indexes are those of stem_ar_encode_image.
namespace {

struct WSegB {
    const float *x;      // image 0
    int len, woff;
    long sh, sw, sp;
    long sg;             // floats between consecutive images
};

constexpr int WAVE_ROWS_B = 32;   // workgroup rows over which the G * np positions of a step are spread
constexpr int WAVE_U = 4;         // positions a wavefront accumulates side by side ...
constexpr int WAVE_R = 4;         // ... for this many output rows

// positions j0, j0 + dj, ..., j0 + (U-1) dj of the step (all < G * np) for the output rows n .. n + WAVE_R - 1: every k step loads
// WAVE_R weight vectors and U x vectors for WAVE_R * U dot products (the single-image kernel loads two vectors per product; at G = 8
// the step is bound by those L1 reads, not by launches)
template <int U>
__device__ __forceinline__ void wave_dots(const float *wr, int ldw, const float (&b)[WAVE_R], const WSegB (&segs)[3], float *y, int ldy, long ygs,
                                          int n, int act, float slope, int lane, int j0, int dj, int np, int h0, int t)
{
    float acc[U][WAVE_R];
    const float *xp[U][3];
    size_t yo[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = j0 + u * dj, g = j / np, p = j - g * np;
        const int h = h0 + p, w = t - 3 * h;
#pragma unroll
        for (int q = 0; q < 3; ++q) xp[u][q] = segs[q].x + segs[q].sg * g + segs[q].sh * h + segs[q].sw * w + segs[q].sp * p;
        yo[u] = (size_t)g * ygs + (size_t)p * ldy + n;
#pragma unroll
        for (int r = 0; r < WAVE_R; ++r) acc[u][r] = 0.f;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const WSegB s = segs[q];
        for (int k = lane * 4; k < s.len; k += 256) {
            f32x4 wv[WAVE_R], xv[U];
#pragma unroll
            for (int r = 0; r < WAVE_R; ++r) wv[r] = *reinterpret_cast<const f32x4 *>(wr + (size_t)r * ldw + s.woff + k);
#pragma unroll
            for (int u = 0; u < U; ++u) xv[u] = *reinterpret_cast<const f32x4 *>(xp[u][q] + k);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int r = 0; r < WAVE_R; ++r) acc[u][r] += dot4(xv[u], wv[r]);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < WAVE_R; ++r) {
            const float a = wave_sum(acc[u][r]);
            if (lane == 0) y[yo[u] + r] = finish(a, b[r], act, slope);
        }
}

// N % WAVE_R == 0 (the entry point checks it): a wavefront's WAVE_R rows are all inside the matrix
__global__ __launch_bounds__(256) void gemv3_wave_batch_kernel(const float *W, int ldw, const float *bias, WSegB s0, WSegB s1, WSegB s2,
                                                               float *y, int ldy, long ygs, int N, int act, float slope, int t, int H, int Wd,
                                                               int G)
{
    const int lane = threadIdx.x & 63;
    const int n = (blockIdx.x * 4 + (threadIdx.x >> 6)) * WAVE_R;
    if (n >= N) return;
    int h0, np;
    wave_range(t, H, Wd, h0, np);
    const int total = G * np, dj = gridDim.y;
    const float *wr = W + (size_t)n * ldw;
    float b[WAVE_R];
#pragma unroll
    for (int r = 0; r < WAVE_R; ++r) b[r] = bias ? bias[n + r] : 0.f;
    const WSegB segs[3] = {s0, s1, s2};
    int j = blockIdx.y;
    for (; j + (WAVE_U - 1) * dj < total; j += WAVE_U * dj) wave_dots<WAVE_U>(wr, ldw, b, segs, y, ldy, ygs, n, act, slope, lane, j, dj, np, h0, t);
    for (; j + dj < total; j += 2 * dj) wave_dots<2>(wr, ldw, b, segs, y, ldy, ygs, n, act, slope, lane, j, dj, np, h0, t);
    for (; j < total; j += dj) wave_dots<1>(wr, ldw, b, segs, y, ldy, ygs, n, act, slope, lane, j, dj, np, h0, t);
}

__global__ void ar_finish_encode_wave_batch_kernel(const float *gp, long gps, const float *table, int T, float scale_bound, float *buf, long bufs,
                                                   int32_t *sym, int32_t *idx, int M, int t, int H, int Wd, int Wp, int pad, int G)
{
    WaveElem e;
    if (!wave_elem(blockIdx.x * blockDim.x + threadIdx.x, t, H, Wd, M, G, e)) return;
    const float *gpp = gp + (size_t)e.g * gps + (size_t)e.p * 2 * M;
    const float mu = gpp[M + e.c];
    const int k = scale_index(gpp[e.c], scale_bound, table, T);
    float *pix = buf + (size_t)e.g * bufs + ((size_t)(e.h + pad) * Wp + (e.w + pad)) * M;
    float q;
    pix[e.c] = quantise(pix[e.c], mu, q);
    const size_t o = (((size_t)e.g * H + e.h) * Wd + e.w) * M + e.c;
    sym[o] = (int32_t)q;
    idx[o] = k;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the arguments stem_ar_encode_batch and stem_ar_decode_wave_batch have in common, in the order of their prototypes
struct WaveBatchArgs {
    const float *w_ctx; int ld_ctx; const float *b_ctx, *w0; int ld0; const float *b0; int n0;
    const float *w1; int ld1; const float *b1; int n1; const float *w2; int ld2; const float *b2;
    float *buf; int G, H, W, M, pad; const float *tp, *hp;
    float *wctx, *wh1, *wh2, *wgp; const float *table; int T; float scale_bound, slope;
    int maxp() const { return H < (W + 2) / 3 ? H : (W + 2) / 3; }       // positions of the largest step
};

// The checks the two entry points share, under the name `who` of the one that asks.  `own`: the pointers only that entry point takes are
// there; `boxes_ok`: its host mailboxes (the decoder's) are aligned.
int wave_batch_check(const char *who, const WaveBatchArgs &a, bool own, bool boxes_ok)
{
    STEM_CHECK_ARG(a.w_ctx && a.b_ctx && a.w0 && a.b0 && a.w1 && a.b1 && a.w2 && a.b2 && a.buf && a.hp && a.wctx && a.wh1 && a.wh2 && a.wgp && a.table && own,
                   "%s: null pointer", who);
    STEM_CHECK_ARG(a.G >= 1, "%s: at least one image per call, got %d", who, a.G);
    static_assert(WAVE_R == 4, "the size check below is what keeps a wavefront's WAVE_R rows inside each matrix (2M, n0, n1)");
    STEM_CHECK_ARG(a.H > 0 && a.W > 0 && a.M > 0 && a.M % 4 == 0 && a.n0 > 0 && a.n1 > 0 && a.n0 % 4 == 0 && a.n1 % 4 == 0 && a.ld_ctx % 4 == 0 &&
                   a.ld0 % 4 == 0 && a.ld1 % 4 == 0 && a.ld2 % 4 == 0 && a.T >= 1 && a.pad == 2, "%s: bad sizes", who);
    STEM_CHECK_ARG(aligned16(a.w_ctx) && aligned16(a.w0) && aligned16(a.w1) && aligned16(a.w2) && aligned16(a.buf) && aligned16(a.tp) && aligned16(a.hp) &&
                   aligned16(a.wctx) && aligned16(a.wh1) && aligned16(a.wh2) && aligned16(a.wgp), "%s: weights, buf, tp, hp and scratch must be 16-byte aligned", who);
    STEM_CHECK_ARG(boxes_ok, "%s: the mailboxes must be 4-byte aligned", who);
    STEM_CHECK_ARG((long)a.G * a.maxp() * a.M <= 0x7fffffffL, "%s: G * positions per step * M = %ld does not fit an int", who, (long)a.G * a.maxp() * a.M);
    return 0;
}

// Step t (np > 0 positions per image) of G images: the four products ctx, EPM.0, EPM.2, EPM.4 over the step's G * np positions, into the
// scratch [G][maxp][2M | n0 | n1 | 2M].  The encoder queues this and then quantises; the wavefront decoder queues the same and then
// asks the host for the symbols -- one function, so the decoder's entropy parameters are the encoder's by construction.
void wave_step_products(const WaveBatchArgs &a, hipStream_t st, int t, int np)
{
    const int M = a.M, P = 2 * M, n0 = a.n0, n1 = a.n1, maxp = a.maxp();
    const long row = (long)(a.W + 2 * a.pad) * M;
    const long bufs = (long)(a.H + 2 * a.pad) * row, pris = (long)a.H * a.W * P;    // image strides of buf and of tp / hp
    const WSegB none{nullptr, 0, 0, 0, 0, 0, 0};
    // context window of position (h, w): rows h, h+1 (5 pixels) and h+2 (2 pixels) of the image's padded buffer, starting at column w
    const WSegB c0{a.buf, 5 * M, 0, row, M, 0, bufs}, c1{a.buf + row, 5 * M, 5 * M, row, M, 0, bufs}, c2{a.buf + 2 * row, 2 * M, 10 * M, row, M, 0, bufs};
    const WSegB sctx{a.wctx, P, a.tp ? 2 * P : P, 0, 0, P, (long)maxp * P};
    const WSegB stp{a.tp, P, 0, (long)a.W * P, P, 0, pris}, shp{a.hp, P, a.tp ? P : 0, (long)a.W * P, P, 0, pris};
    const WSegB sh1{a.wh1, n0, 0, 0, 0, n0, (long)maxp * n0}, sh2{a.wh2, n1, 0, 0, 0, n1, (long)maxp * n1};
    const int total = a.G * np;
    const int gy = total < WAVE_ROWS_B ? total : WAVE_ROWS_B;
    auto product = [&](const float *Wm, int ldw, const float *bias, const WSegB &s0, const WSegB &s1, const WSegB &s2, float *y, int N, int act) {
        hipLaunchKernelGGL(gemv3_wave_batch_kernel, dim3(cdiv(N, 4 * WAVE_R), gy), dim3(256), 0, st, Wm, ldw, bias, s0, s1, s2, y, N, (long)maxp * N, N, act,
                           act ? a.slope : 0.f, t, a.H, a.W, a.G);
    };
    product(a.w_ctx, a.ld_ctx, a.b_ctx, c0, c1, c2, a.wctx, P, 0);
    if (a.tp) product(a.w0, a.ld0, a.b0, stp, shp, sctx, a.wh1, n0, (int)STEM_ACT_LRELU);
    else product(a.w0, a.ld0, a.b0, shp, sctx, none, a.wh1, n0, (int)STEM_ACT_LRELU);
    product(a.w1, a.ld1, a.b1, sh1, none, none, a.wh2, n1, (int)STEM_ACT_LRELU);
    product(a.w2, a.ld2, a.b2, sh2, none, none, a.wgp, P, 0);
}

}   // namespace

STEM_EXPORT int stem_ar_encode_batch(const float *w_ctx, int ld_ctx, const float *b_ctx, const float *w0, int ld0, const float *b0, int n0,
                                     const float *w1, int ld1, const float *b1, int n1, const float *w2, int ld2, const float *b2,
                                     float *buf, int G, int H, int W, int M, int pad, const float *tp, const float *hp,
                                     float *wctx, float *wh1, float *wh2, float *wgp, const float *table, int T, float scale_bound,
                                     float slope, int32_t *sym, int32_t *idx, void *stream)
{
    const WaveBatchArgs a{w_ctx, ld_ctx, b_ctx, w0, ld0, b0, n0, w1, ld1, b1, n1, w2, ld2, b2, buf, G, H, W, M, pad, tp, hp,
                          wctx, wh1, wh2, wgp, table, T, scale_bound, slope};
    if (int rc = wave_batch_check("stem_ar_encode_batch", a, sym && idx, true)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int P = 2 * M, Wp = W + 2 * pad;
    const long bufs = (long)(H + 2 * pad) * Wp * M, gps = (long)a.maxp() * P;        // image strides of buf and of wgp
    for (int t = 0; t < W + 3 * (H - 1); ++t) {
        int h0, np;
        wave_range(t, H, W, h0, np);
        if (np <= 0) continue;                   // W < 3: steps between two rows hold no position
        wave_step_products(a, st, t, np);
        hipLaunchKernelGGL(ar_finish_encode_wave_batch_kernel, dim3(cdiv(G * np * M, 256)), dim3(256), 0, st, wgp, gps, table, T, scale_bound,
                           buf, bufs, sym, idx, M, t, H, W, Wp, pad, G);
    }
    STEM_LAUNCH_CHECK("ar_encode_batch");
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// WAVEFRONT SYMBOL ORDER (include/stem_ar_batch.h states it).  The raster-order decoders above are bound by the count of sequential
// steps, H * W, and that count belongs to the order of the symbols in the stream, not to the model: coded step by step (t = w + 3h, rows
// ascending inside a step, channels inside a position) the decoder needs W + 3(H-1) host round trips -- 321 instead of 8160 for a 1080p
// frame -- and every input of the encoder's wavefront products is already decoded when step t starts.  So the decoder below runs the
// encoder's own launches (wave_step_products, the function stem_ar_encode_batch calls): no float can differ from the encoder's.
namespace {

// one workgroup per raster position and image: the M symbols and the M indexes of the position move to its wavefront rank
__global__ __launch_bounds__(64) void ar_to_wave_order_kernel(const int32_t *sym_r, const int32_t *idx_r, int32_t *sym_w, int32_t *idx_w,
                                                              int H, int Wd, int M)
{
    const int pos = blockIdx.x, g = blockIdx.y;
    const int h = pos / Wd, w = pos - h * Wd, t = w + 3 * h;
    int h0, np;
    wave_range(t, H, Wd, h0, np);
    const size_t img = (size_t)g * H * Wd * M;
    const size_t src = img + (size_t)pos * M, dst = img + (size_t)(wave_positions_before(t, H, Wd) + (h - h0)) * M;
    for (int c = threadIdx.x; c < M; c += blockDim.x) {
        sym_w[dst + c] = sym_r[src + c];
        idx_w[dst + c] = idx_r[src + c];
    }
}

// step t of G images: index = build_indexes(scale) of the step's positions, in wavefront order per image, into the pinned mailbox
__global__ void ar_index_wave_batch_kernel(const float *gp, long gps, const float *table, int T, float scale_bound, int32_t *idx, long idxs,
                                           int M, int t, int H, int Wd, int G)
{
    WaveElem e;
    if (!wave_elem(blockIdx.x * blockDim.x + threadIdx.x, t, H, Wd, M, G, e)) return;
    idx[(size_t)e.g * idxs + (size_t)e.p * M + e.c] = scale_index(gp[(size_t)e.g * gps + (size_t)e.p * 2 * M + e.c], scale_bound, table, T);
}

// step t of G images: buffer <- symbol + mean (symbols from the pinned mailbox, means from the step's wgp)
__global__ void ar_finish_decode_wave_batch_kernel(const float *gp, long gps, const int32_t *sym, long syms, float *buf, long bufs, int M,
                                                   int t, int H, int Wd, int Wp, int pad, int G)
{
    WaveElem e;
    if (!wave_elem(blockIdx.x * blockDim.x + threadIdx.x, t, H, Wd, M, G, e)) return;
    float *pix = buf + (size_t)e.g * bufs + ((size_t)(e.h + pad) * Wp + (e.w + pad)) * M;
    pix[e.c] = dequantise(sym[(size_t)e.g * syms + (size_t)e.p * M + e.c], gp[(size_t)e.g * gps + (size_t)e.p * 2 * M + M + e.c]);
}

}   // namespace

STEM_EXPORT int stem_ar_to_wave_order(const int32_t *sym_raster, const int32_t *idx_raster, int32_t *sym_wave, int32_t *idx_wave, int G, int H,
                                      int W, int M, void *stream)
{
    STEM_CHECK_ARG(sym_raster && idx_raster && sym_wave && idx_wave, "stem_ar_to_wave_order: null pointer");
    STEM_CHECK_ARG(G >= 1 && G <= 65535 && H > 0 && W > 0 && M > 0 && (long)H * W <= 0x7fffffffL, "stem_ar_to_wave_order: bad sizes (G=%d H=%d W=%d M=%d)",
                   G, H, W, M);
    STEM_CHECK_ARG(sym_raster != sym_wave && idx_raster != idx_wave && sym_wave != idx_wave, "stem_ar_to_wave_order: source and destination overlap");
    hipLaunchKernelGGL(ar_to_wave_order_kernel, dim3(H * W, G), dim3(64), 0, (hipStream_t)stream, sym_raster, idx_raster, sym_wave, idx_wave, H, W, M);
    STEM_LAUNCH_CHECK("ar_to_wave_order");
    return 0;
}

STEM_EXPORT int stem_ar_decode_wave_batch(const float *w_ctx, int ld_ctx, const float *b_ctx, const float *w0, int ld0, const float *b0, int n0,
                                          const float *w1, int ld1, const float *b1, int n1, const float *w2, int ld2, const float *b2,
                                          float *buf, int G, int H, int W, int M, int pad, const float *tp, const float *hp,
                                          float *wctx, float *wh1, float *wh2, float *wgp, const float *table, int T, float scale_bound, float slope,
                                          int32_t *idx_host, int32_t *sym_host, stem_wave_symbol_decoder_fn decode, void *const *decs,
                                          const int32_t *cdfs, int ncdf, int cdf_stride, const int32_t *sizes, const int32_t *offsets, void *stream)
{
    const WaveBatchArgs a{w_ctx, ld_ctx, b_ctx, w0, ld0, b0, n0, w1, ld1, b1, n1, w2, ld2, b2, buf, G, H, W, M, pad, tp, hp,
                          wctx, wh1, wh2, wgp, table, T, scale_bound, slope};
    if (int rc = wave_batch_check("stem_ar_decode_wave_batch", a, idx_host && sym_host && decode && decs,
                                  (((uintptr_t)idx_host | (uintptr_t)sym_host) & 3) == 0))
        return rc;
    for (int g = 0; g < G; ++g) STEM_CHECK_ARG(decs[g], "stem_ar_decode_wave_batch: no decoder handle for image %d", g);
    hipStream_t st = (hipStream_t)stream;
    const int P = 2 * M, Wp = W + 2 * pad;
    const long bufs = (long)(H + 2 * pad) * Wp * M;                                  // image stride of buf
    const long gps = (long)a.maxp() * P, boxs = (long)a.maxp() * M;                  // ... of wgp and of the mailboxes
    StepTimer tm;
    // buffer <- symbol + mean for the step whose symbols sit in the mailbox
    auto commit = [&](int t) {
        int h0, np;
        wave_range(t, H, W, h0, np);
        hipLaunchKernelGGL(ar_finish_decode_wave_batch_kernel, dim3(cdiv(G * np * M, 256)), dim3(256), 0, st, wgp, gps, sym_host, boxs, buf, bufs, M,
                           t, H, W, Wp, pad, G);
    };
    int t_prev = -1, steps = 0;               // the step whose symbols sit in the mailbox, not yet committed to buf
    for (int t = 0; t < W + 3 * (H - 1); ++t) {
        int h0, np;
        wave_range(t, H, W, h0, np);
        if (np <= 0) continue;                   // W < 3: steps between two rows hold no position
        tm.at(0);
        if (t_prev >= 0) commit(t_prev);
        wave_step_products(a, st, t, np);        // the encoder's launches
        hipLaunchKernelGGL(ar_index_wave_batch_kernel, dim3(cdiv(G * np * M, 256)), dim3(256), 0, st, wgp, gps, table, T, scale_bound, idx_host, boxs, M,
                           t, H, W, G);
        tm.at(1);
        if (hipStreamSynchronize(st) != hipSuccess) {
            stem_set_error("stem_ar_decode_wave_batch: device error at step %d: %s", t, hipGetErrorString(hipGetLastError()));
            return -2;
        }
        tm.at(2);
        for (int g = 0; g < G; ++g)
            if (int rc = decode(decs[g], idx_host + (size_t)g * boxs, (size_t)np * M, cdfs, ncdf, cdf_stride, sizes, offsets, sym_host + (size_t)g * boxs)) {
                stem_set_error("stem_ar_decode_wave_batch: host symbol decoder failed (%d) for image %d at step %d", rc, g, t);
                return -3;
            }
        t_prev = t;
        ++steps;
        tm.step_done();
    }
    if (tm.on)
        fprintf(stderr, "[ar decode wave batch] G=%d steps=%d positions=%d: launch %.1f us, wait %.1f us, host coder %.1f us per step\n", G, steps, H * W,
                tm.launch / steps, tm.wait / steps, tm.host / steps);
    commit(t_prev);
    STEM_LAUNCH_CHECK("ar_decode_wave_batch");
    if (hipStreamSynchronize(st) != hipSuccess) {             // the last step read the mailbox: the caller may free it on return
        stem_set_error("stem_ar_decode_wave_batch: device error after the last step: %s", hipGetErrorString(hipGetLastError()));
        return -2;
    }
    return 0;
}
