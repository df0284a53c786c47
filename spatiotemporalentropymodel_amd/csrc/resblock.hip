// Device operations of the residual / sub-pixel / attention blocks of the cheng2020 I-frame models, compressai/layers/layers.py:
//   pixel shuffle: nn.PixelShuffle(r) in NHWC, with the leaky ReLU and the `out += identity` that follow it in
//                  ResidualBlockUpsample folded in                                             (layers.py:55-59, 118-126)
//   add_act:       ResidualUnit's relu(conv(x) + x)                                            (layers.py:191-196)
//   gate:          AttentionBlock's a * sigmoid(b) + x                                         (layers.py:207-213)
// All fp32 NHWC with an explicit pixel pitch per tensor (channel-slice views need no copy), all HBM-bound, no atomics: every output
// element has exactly one writer.  Channel counts that are multiples of 4 take 16-byte accesses on both sides.
//
// The shuffle moves, per input pixel, a run of C*r*r floats to r runs of r*C floats (one per output row).  A workgroup takes one
// segment of an input row (tw pixels) and a chunk of cc output channels, reads its cc*r*r floats per pixel with 16-byte loads,
// scatters them into LDS in OUTPUT order ([i][w][j][c]: 4-byte LDS writes), and after a barrier streams the r output rows out of
// LDS with 16-byte reads and stores -- the addend joins there, with 16-byte loads of its own.  The backward pass is the same
// kernel run the other way round (copy the r gradient rows into LDS, gather per input float4).
//
// Stated bit for bit (tests/cheng_ref.py): products and sums are single roundings, no contraction into FMAs.
#include "stem_common.h"
#include "../../include/stem_blocks.h"

#pragma clang fp contract(off)

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_LDS_FLOATS = 12288;      // 48 KiB of LDS per workgroup: three workgroups per CU
constexpr int PS_MAX_TW = 64;

__device__ inline float lrelu(float v, float slope) { return v > 0.f ? v : __fmul_rn(v, slope); }

struct PsGeom {
    int B, H, W, C, r, rr;
    int ldi, ldo, lda;                    // pixel pitches: shuffle input side, output side, addend (forward only)
    int TW, nseg, cc;                     // pixels per segment, segments per row, output channels per chunk (a multiple of 4)
};

// blockIdx.x: (b * H + h) * nseg + segment; blockIdx.y: channel chunk
template <bool BWD>
__global__ __launch_bounds__(PS_THREADS) void pixel_shuffle_vec_kernel(const float *__restrict__ in, const float *__restrict__ addend,
                                                                        const float *__restrict__ dout, float *__restrict__ out, PsGeom g,
                                                                        float slope)
{
    extern __shared__ __attribute__((aligned(16))) float ps_lds[];
    const int seg = blockIdx.x % g.nseg;
    const size_t row = blockIdx.x / g.nseg;                       // b * H + h
    const int w0 = seg * g.TW, tw = min(g.TW, g.W - w0);
    const int c0 = blockIdx.y * g.cc, cc = min(g.cc, g.C - c0);   // C % 4 == 0 and g.cc % 4 == 0, so cc % 4 == 0
    const int r = g.r, rr = g.rr;
    const int nin4 = cc * rr / 4;                                 // float4 per input pixel in this chunk
    const int cc4 = cc / 4, rowv = tw * r * cc4;                  // float4 per output pixel / per output row of the segment
    const size_t ipix0 = row * g.W + w0;                          // first input pixel
    const size_t b = row / g.H, h = row % g.H;
    const size_t OW = (size_t)g.W * r;
    // float4 v of the segment's r output rows (LDS order) -> its place in the output-side tensor of pitch ld
    auto oaddr = [&](int v, int ld) -> size_t {
        const int i = v / rowv, rem = v % rowv, p = rem / cc4, c4 = rem % cc4;
        return (((b * g.H + h) * r + i) * OW + (size_t)w0 * r + p) * ld + c0 + c4 * 4;
    };
    // element k of a pixel's chunk (k = (c - c0) * rr + i * r + j) at pixel w of the segment -> LDS float index
    auto lidx = [&](int w, int k) -> int {
        const int c = k / rr, rem = k % rr, i = rem / r, j = rem % r;
        return ((i * tw + w) * r + j) * cc + c;
    };
    if (!BWD) {
        for (int v = threadIdx.x; v < tw * nin4; v += PS_THREADS) {
            const int w = v / nin4, q = v % nin4;
            const f32x4 x = *reinterpret_cast<const f32x4 *>(in + (ipix0 + w) * g.ldi + (size_t)c0 * rr + q * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) ps_lds[lidx(w, q * 4 + e)] = lrelu(x[e], slope);
        }
        __syncthreads();
        for (int v = threadIdx.x; v < r * rowv; v += PS_THREADS) {
            f32x4 y = reinterpret_cast<const f32x4 *>(ps_lds)[v];
            if (addend) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(addend + oaddr(v, g.lda));
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = __fadd_rn(y[e], a[e]);
            }
            *reinterpret_cast<f32x4 *>(out + oaddr(v, g.ldo)) = y;
        }
    } else {
        for (int v = threadIdx.x; v < r * rowv; v += PS_THREADS)
            reinterpret_cast<f32x4 *>(ps_lds)[v] = *reinterpret_cast<const f32x4 *>(dout + oaddr(v, g.ldo));
        __syncthreads();
        for (int v = threadIdx.x; v < tw * nin4; v += PS_THREADS) {
            const int w = v / nin4, q = v % nin4;
            const size_t off = (size_t)c0 * rr + q * 4;
            f32x4 d;
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = ps_lds[lidx(w, q * 4 + e)];
            if (in) {
                const f32x4 x = *reinterpret_cast<const f32x4 *>(in + (ipix0 + w) * g.ldi + off);
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = x[e] > 0.f ? d[e] : __fmul_rn(d[e], slope);
            }
            *reinterpret_cast<f32x4 *>(out + (ipix0 + w) * g.lda + off) = d;          // backward: lda is din's pitch
        }
    }
}

// any C (the 3 image channels behind g_s): one thread per OUTPUT element (forward) / per INPUT-side element (backward); adjacent
// lanes write adjacent floats, the strided side stays inside the cache lines of one pixel run
template <bool BWD>
__global__ __launch_bounds__(256) void pixel_shuffle_direct_kernel(const float *__restrict__ in, const float *__restrict__ addend,
                                                                    const float *__restrict__ dout, float *__restrict__ out, PsGeom g,
                                                                    float slope, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int r = g.r, rr = g.rr;
    const size_t OW = (size_t)g.W * r, OH = (size_t)g.H * r;
    if (!BWD) {
        const int c = (int)(idx % g.C);
        size_t p = idx / g.C;
        const size_t ow = p % OW;
        p /= OW;
        const size_t oh = p % OH, b = p / OH;
        const size_t ipix = (b * g.H + oh / r) * g.W + ow / r, opix = (b * OH + oh) * OW + ow;
        float y = lrelu(in[ipix * g.ldi + (size_t)c * rr + (oh % r) * r + ow % r], slope);
        if (addend) y = __fadd_rn(y, addend[opix * g.lda + c]);
        out[opix * g.ldo + c] = y;
    } else {
        const size_t crr = (size_t)g.C * rr;
        const int k = (int)(idx % crr);
        const size_t ipix = idx / crr;
        const size_t w = ipix % g.W, bh = ipix / g.W, h = bh % g.H, b = bh / g.H;
        const int c = k / rr, rem = k % rr, i = rem / r, j = rem % r;
        float d = dout[((b * OH + h * r + i) * OW + w * r + j) * g.ldo + c];
        if (in) d = in[ipix * g.ldi + k] > 0.f ? d : __fmul_rn(d, slope);
        out[ipix * g.lda + k] = d;
    }
}

// ---- the elementwise operations: n = npix * C (scalar) or npix * C / 4 (16-byte) items, item -> (pixel, channel offset) ---------
template <typename T>
struct Pitched {
    const float *p;
    int ld;
    __device__ T load(size_t pix, int c) const { return *reinterpret_cast<const T *>(p + pix * ld + c); }
};
template <typename T>
__device__ inline void pstore(float *p, int ld, size_t pix, int c, T v) { *reinterpret_cast<T *>(p + pix * ld + c) = v; }

template <typename T> struct lanes { static constexpr int n = 4; };
template <> struct lanes<float> { static constexpr int n = 1; };
__device__ inline float &el(float &v, int) { return v; }
__device__ inline float &el(f32x4 &v, int e) { return reinterpret_cast<float *>(&v)[e]; }

template <typename T>
__global__ __launch_bounds__(256) void add_act_fwd_kernel(Pitched<T> a, Pitched<T> b, float *out, int ldo, size_t n, int cw, float slope)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t pix = i / cw;
    const int c = (int)(i % cw) * lanes<T>::n;
    T av = a.load(pix, c), bv = b.load(pix, c), o;
#pragma unroll
    for (int e = 0; e < lanes<T>::n; ++e) el(o, e) = lrelu(__fadd_rn(el(av, e), el(bv, e)), slope);
    pstore<T>(out, ldo, pix, c, o);
}

template <typename T>
__global__ __launch_bounds__(256) void add_act_bwd_kernel(Pitched<T> out, Pitched<T> dout, float *dab, int ldg, size_t n, int cw, float slope)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t pix = i / cw;
    const int c = (int)(i % cw) * lanes<T>::n;
    T ov = out.load(pix, c), dv = dout.load(pix, c), g;
#pragma unroll
    for (int e = 0; e < lanes<T>::n; ++e) el(g, e) = el(ov, e) > 0.f ? el(dv, e) : __fmul_rn(el(dv, e), slope);
    pstore<T>(dab, ldg, pix, c, g);
}

// s = sigmoid(b) and 1 - s, both to a few ulp at every b: e = exp(-|b|) <= 1 never overflows, and the smaller of the two is
// e / (1 + e), not a difference of nearly equal numbers
__device__ inline void sigmoid_pair(float b, float &s, float &one_minus_s)
{
    const float e = expf(-fabsf(b));
    const float d = __fadd_rn(1.f, e);
    const float big = __fdiv_rn(1.f, d), small = __fdiv_rn(e, d);
    s = b >= 0.f ? big : small;
    one_minus_s = b >= 0.f ? small : big;
}

template <typename T>
__global__ __launch_bounds__(256) void gate_fwd_kernel(Pitched<T> a, Pitched<T> b, Pitched<T> x, float *out, int ldo, size_t n, int cw)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t pix = i / cw;
    const int c = (int)(i % cw) * lanes<T>::n;
    T av = a.load(pix, c), bv = b.load(pix, c), xv = x.load(pix, c), o;
#pragma unroll
    for (int e = 0; e < lanes<T>::n; ++e) {
        float s, t;
        sigmoid_pair(el(bv, e), s, t);
        el(o, e) = __fadd_rn(__fmul_rn(el(av, e), s), el(xv, e));
    }
    pstore<T>(out, ldo, pix, c, o);
}

template <typename T>
__global__ __launch_bounds__(256) void gate_bwd_kernel(Pitched<T> a, Pitched<T> b, Pitched<T> dout, float *da, int ldda, float *db, int lddb,
                                                       size_t n, int cw)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t pix = i / cw;
    const int c = (int)(i % cw) * lanes<T>::n;
    T av = a.load(pix, c), bv = b.load(pix, c), dv = dout.load(pix, c), ga, gb;
#pragma unroll
    for (int e = 0; e < lanes<T>::n; ++e) {
        float s, t;
        sigmoid_pair(el(bv, e), s, t);
        el(ga, e) = __fmul_rn(el(dv, e), s);
        el(gb, e) = __fmul_rn(__fmul_rn(__fmul_rn(el(dv, e), el(av, e)), s), t);
    }
    pstore<T>(da, ldda, pix, c, ga);
    pstore<T>(db, lddb, pix, c, gb);
}

inline bool al16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// a tensor argument of `C` channels and pixel pitch `ld`: the pitch covers the channels; on the 16-byte path (`vec`: the
// operation's channel count is a multiple of 4) the pitch is a multiple of 4 floats and the base 16-byte aligned.  0 if fine
// (null pointers are checked by the caller).
int check_tensor(const char *fn, const char *name, const void *p, int ld, long long C, bool vec)
{
    STEM_CHECK_ARG(ld >= C, "%s: pitch of %s (%d) is smaller than its %lld channels", fn, name, ld, C);
    if (vec) {
        STEM_CHECK_ARG(ld % 4 == 0, "%s: pitch of %s (%d) is not a multiple of 4 on the 16-byte path (C %% 4 == 0)", fn, name, ld);
        STEM_CHECK_ARG(al16(p), "%s: %s is not 16-byte aligned on the 16-byte path (C %% 4 == 0)", fn, name);
    }
    return 0;
}
#define CHECK_TENSOR(fn, name, p, ld, C, vec)                          \
    do {                                                               \
        if (check_tensor(fn, name, p, ld, C, vec) != 0) return -1;     \
    } while (0)

int elementwise_dims(const char *fn, size_t npix, int C, size_t &n, int &cw)
{
    STEM_CHECK_ARG(C >= 1, "%s: C = %d, need at least one channel", fn, C);
    cw = C % 4 == 0 ? C / 4 : C;
    n = npix * (size_t)cw;
    STEM_CHECK_ARG(cdivz(n, 256) <= 0x7FFFFFFFull, "%s: %zu pixels of %d channels exceed one grid", fn, npix, C);
    return 0;
}

// shape checks shared by the two directions of the shuffle; fills g (without the pitches)
int shuffle_geom(const char *fn, int B, int H, int W, int C, int r, PsGeom &g)
{
    STEM_CHECK_ARG(r >= 1, "%s: r = %d, the up-sampling factor is at least 1", fn, r);
    STEM_CHECK_ARG(C >= 1, "%s: C = %d, need at least one output channel", fn, C);
    STEM_CHECK_ARG(B >= 0 && H >= 0 && W >= 0, "%s: bad dims B=%d H=%d W=%d", fn, B, H, W);
    STEM_CHECK_ARG((long long)r * r * C <= 0x7FFFFFFF && (long long)W * r <= 0x7FFFFFFF && (long long)H * r <= 0x7FFFFFFF,
                   "%s: C * r * r = %lld input channels / %lld x %lld output pixels exceed int", fn, (long long)r * r * C, (long long)H * r,
                   (long long)W * r);
    g.B = B, g.H = H, g.W = W, g.C = C, g.r = r, g.rr = r * r;
    g.TW = g.nseg = g.cc = 0;
    return 0;
}

// the LDS kernel serves C % 4 == 0 as long as a 4-channel chunk of one pixel fits its LDS; everything else is the direct kernel
bool shuffle_plan_vec(PsGeom &g)
{
    if (g.C % 4 != 0 || (long long)g.rr * 4 > PS_LDS_FLOATS) return false;
    const long long per_pixel = (long long)g.C * g.rr;
    if (per_pixel <= PS_LDS_FLOATS) {
        g.cc = g.C;
        g.TW = (int)(PS_LDS_FLOATS / per_pixel);
        if (g.TW > PS_MAX_TW) g.TW = PS_MAX_TW;
        if (g.TW > g.W) g.TW = g.W;
    } else {
        g.cc = (PS_LDS_FLOATS / g.rr) & ~3;
        g.TW = 1;
    }
    g.nseg = cdiv(g.W, g.TW);
    return true;
}

template <bool BWD>
int shuffle_launch(const char *fn, const float *in, const float *addend, const float *dout, float *out, PsGeom g, float slope, void *stream)
{
    const size_t in_elems = (size_t)g.B * g.H * g.W * g.C * g.rr;
    if (in_elems == 0) return 0;
    if (shuffle_plan_vec(g)) {
        const size_t gx = (size_t)g.B * g.H * g.nseg;
        const int gy = cdiv(g.C, g.cc);
        STEM_CHECK_ARG(gx <= 0x7FFFFFFFull && gy <= 65535, "%s: %zu row segments x %d channel chunks exceed one grid", fn, gx, gy);
        const size_t lds = (size_t)g.TW * g.cc * g.rr * sizeof(float);
        hipLaunchKernelGGL(pixel_shuffle_vec_kernel<BWD>, dim3((unsigned)gx, (unsigned)gy), dim3(PS_THREADS), lds, (hipStream_t)stream, in,
                           addend, dout, out, g, slope);
    } else {
        STEM_CHECK_ARG(cdivz(in_elems, 256) <= 0x7FFFFFFFull, "%s: %zu elements exceed one grid", fn, in_elems);
        hipLaunchKernelGGL(pixel_shuffle_direct_kernel<BWD>, dim3((unsigned)cdivz(in_elems, 256)), dim3(256), 0, (hipStream_t)stream, in,
                           addend, dout, out, g, slope, in_elems);
    }
    STEM_LAUNCH_CHECK(fn);
    return 0;
}

}   // namespace

STEM_EXPORT int stem_pixel_shuffle_fwd(const float *in, int ldi, const float *addend, int lda, float *out, int ldo, int B, int H, int W, int C,
                                       int r, float slope, void *stream)
{
    const char *fn = "stem_pixel_shuffle_fwd";
    STEM_CHECK_ARG(in && out, "%s: null pointer", fn);
    PsGeom g;
    if (shuffle_geom(fn, B, H, W, C, r, g) != 0) return -1;
    CHECK_TENSOR(fn, "in", in, ldi, (long long)C * r * r, C % 4 == 0);
    CHECK_TENSOR(fn, "out", out, ldo, C, C % 4 == 0);
    if (addend) CHECK_TENSOR(fn, "addend", addend, lda, C, C % 4 == 0);
    g.ldi = ldi, g.ldo = ldo, g.lda = addend ? lda : 0;
    return shuffle_launch<false>(fn, in, addend, nullptr, out, g, slope, stream);
}

STEM_EXPORT int stem_pixel_shuffle_bwd(const float *in, int ldi, const float *dout, int ldo, float *din, int ldd, int B, int H, int W, int C,
                                       int r, float slope, void *stream)
{
    const char *fn = "stem_pixel_shuffle_bwd";
    STEM_CHECK_ARG(dout && din, "%s: null pointer", fn);
    STEM_CHECK_ARG(in || slope == 1.f, "%s: null in (the forward input) with an activation of slope %g", fn, (double)slope);
    PsGeom g;
    if (shuffle_geom(fn, B, H, W, C, r, g) != 0) return -1;
    if (in) CHECK_TENSOR(fn, "in", in, ldi, (long long)C * r * r, C % 4 == 0);
    CHECK_TENSOR(fn, "dout", dout, ldo, C, C % 4 == 0);
    CHECK_TENSOR(fn, "din", din, ldd, (long long)C * r * r, C % 4 == 0);
    g.ldi = in ? ldi : 0, g.ldo = ldo, g.lda = ldd;
    return shuffle_launch<true>(fn, in, nullptr, dout, din, g, slope, stream);
}

#define ELEMENTWISE_LAUNCH(kernel, fn, ...)                                                                                      \
    do {                                                                                                                         \
        if (n == 0) return 0;                                                                                                    \
        if (C % 4 == 0)                                                                                                          \
            hipLaunchKernelGGL(kernel<f32x4>, dim3((unsigned)cdivz(n, 256)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);    \
        else                                                                                                                     \
            hipLaunchKernelGGL(kernel<float>, dim3((unsigned)cdivz(n, 256)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);    \
        STEM_LAUNCH_CHECK(fn);                                                                                                   \
        return 0;                                                                                                                \
    } while (0)

STEM_EXPORT int stem_add_act_fwd(const float *a, int lda, const float *b, int ldb, float *out, int ldo, size_t npix, int C, float slope,
                                 void *stream)
{
    const char *fn = "stem_add_act_fwd";
    STEM_CHECK_ARG(a && b && out, "%s: null pointer", fn);
    size_t n;
    int cw;
    if (elementwise_dims(fn, npix, C, n, cw) != 0) return -1;
    CHECK_TENSOR(fn, "a", a, lda, C, C % 4 == 0);
    CHECK_TENSOR(fn, "b", b, ldb, C, C % 4 == 0);
    CHECK_TENSOR(fn, "out", out, ldo, C, C % 4 == 0);
    ELEMENTWISE_LAUNCH(add_act_fwd_kernel, fn, {a, lda}, {b, ldb}, out, ldo, n, cw, slope);
}

STEM_EXPORT int stem_add_act_bwd(const float *out, int ldo, const float *dout, int ldd, float *dab, int ldg, size_t npix, int C, float slope,
                                 void *stream)
{
    const char *fn = "stem_add_act_bwd";
    STEM_CHECK_ARG(out && dout && dab, "%s: null pointer", fn);
    size_t n;
    int cw;
    if (elementwise_dims(fn, npix, C, n, cw) != 0) return -1;
    CHECK_TENSOR(fn, "out", out, ldo, C, C % 4 == 0);
    CHECK_TENSOR(fn, "dout", dout, ldd, C, C % 4 == 0);
    CHECK_TENSOR(fn, "dab", dab, ldg, C, C % 4 == 0);
    ELEMENTWISE_LAUNCH(add_act_bwd_kernel, fn, {out, ldo}, {dout, ldd}, dab, ldg, n, cw, slope);
}

STEM_EXPORT int stem_gate_fwd(const float *a, int lda, const float *b, int ldb, const float *x, int ldx, float *out, int ldo, size_t npix,
                              int C, void *stream)
{
    const char *fn = "stem_gate_fwd";
    STEM_CHECK_ARG(a && b && x && out, "%s: null pointer", fn);
    size_t n;
    int cw;
    if (elementwise_dims(fn, npix, C, n, cw) != 0) return -1;
    CHECK_TENSOR(fn, "a", a, lda, C, C % 4 == 0);
    CHECK_TENSOR(fn, "b", b, ldb, C, C % 4 == 0);
    CHECK_TENSOR(fn, "x", x, ldx, C, C % 4 == 0);
    CHECK_TENSOR(fn, "out", out, ldo, C, C % 4 == 0);
    ELEMENTWISE_LAUNCH(gate_fwd_kernel, fn, {a, lda}, {b, ldb}, {x, ldx}, out, ldo, n, cw);
}

STEM_EXPORT int stem_gate_bwd(const float *a, int lda, const float *b, int ldb, const float *dout, int ldd, float *da, int ldda, float *db,
                              int lddb, size_t npix, int C, void *stream)
{
    const char *fn = "stem_gate_bwd";
    STEM_CHECK_ARG(a && b && dout && da && db, "%s: null pointer", fn);
    size_t n;
    int cw;
    if (elementwise_dims(fn, npix, C, n, cw) != 0) return -1;
    CHECK_TENSOR(fn, "a", a, lda, C, C % 4 == 0);
    CHECK_TENSOR(fn, "b", b, ldb, C, C % 4 == 0);
    CHECK_TENSOR(fn, "dout", dout, ldd, C, C % 4 == 0);
    CHECK_TENSOR(fn, "da", da, ldda, C, C % 4 == 0);
    CHECK_TENSOR(fn, "db", db, lddb, C, C % 4 == 0);
    ELEMENTWISE_LAUNCH(gate_bwd_kernel, fn, {a, lda}, {b, ldb}, {dout, ldd}, da, ldda, db, lddb, n, cw);
}
