// Raw planar YUV 4:2:0 (8- or 10-bit samples, BT.709, full range) <-> fp32 NCHW RGB: the fused forms of the reference's
// transforms (compressai/transforms/functional.py:26-135),
//     stem_yuv420_to_rgb   ycbcr2rgb(yuv_420_to_444((y, u, v) / peak, mode))           :47-65 after :100-135
//     stem_rgb_to_yuv420   yuv_444_to_420(rgb2ycbcr(x)) [-> integer planes, + SSE]     :68-97 after :26-44
// peak = 2^bit_depth - 1.
//
// Both are streaming kernels with one work item = 2 rows x 4 columns of luma = 1 row x 2 columns of chroma.  Work items are
// numbered along the rows of one image, so a 256-thread workgroup covers a strip of 2 rows x 1024 columns (wrapping to the next
// pair of rows in narrower frames) and blockIdx.y is the image: no workgroup straddles two images.  When W % 4 == 0 (every
// common video size) and the planes are aligned, a lane moves its luma as one 4- or 8-byte vector and its fp32 pixels as 16-byte
// vectors; otherwise (W % 4 == 2) the same body runs element by element, with the last item of a row owning two columns.
//
//   yuv -> rgb: fp32.  The 0.25 / 0.75 interpolation of F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) is
//     done on the integer samples, where it is exact in fp32 (sixteenths of numbers below 2^10), in torch's order (columns, then
//     rows) and with torch's border (output row / column 0 is sample 0, the last one is the last sample); then one division by
//     the peak, then ycbcr2rgb in the reference's order: r and b from y, g from them.  The 3 x 4 chroma neighbourhood of an
//     item is read sample by sample through the caches: the chroma planes are a sixth of the bytes this kernel moves.
//   rgb -> yuv: the arithmetic is fp64 (the fp32 inputs are exact there).  A value in [0,1] comes out of at most ten fp64
//     roundings, ~1e-15 absolute; times the peak (<= 1023) that is ~1e-12 of a sample step, so an integer sample differs from
//     rint() of the float64 reference only within ~1e-12 of a half-integer.  The fp32 planes are the fp64 value rounded once.
//     The kernel moves 12 bytes per pixel in and at most 6 out; the fp64 work hides under it.
//     With source planes, each work item also takes the squared differences of its twelve integer samples; a workgroup reduces
//     them in 64-bit integers to its own three slots of the workspace, a second launch (one workgroup per image) sums the slots.
//     Integer sums: exact, so order-free and bit-reproducible; no atomics.
//
// The arithmetic of a work item is stated in yuv_elem.h, which csrc/frameio.hip shares (the same frames inside padded ones).
#include "stem_common.h"
#include "yuv_elem.h"

namespace {

using namespace yuv_elem;

// the work item of this thread
__device__ inline YuvItem yuv_item(int Hc, int W) { return yuv_item_at((long long)blockIdx.x * YUV_THREADS + threadIdx.x, Hc, W); }

template <typename T, bool VEC>
__global__ __launch_bounds__(YUV_THREADS) void yuv420_to_rgb_kernel(const T *__restrict__ yp, const T *__restrict__ up,
                                                                    const T *__restrict__ vp, int H, int W, float peak, int nearest,
                                                                    int clamp01, float *__restrict__ rgb)
{
    const int Hc = H >> 1, Wc = W >> 1;
    const YuvItem it = yuv_item(Hc, W);
    if (!it.live) return;
    const size_t b = blockIdx.y, plane = (size_t)H * W, cplane = (size_t)Hc * Wc;
    yuv420_item_to_rgb<T, VEC, VEC>(yp + b * plane, up + b * cplane, vp + b * cplane, H, W, it, peak, nearest, clamp01, rgb + b * 3 * plane,
                                    (size_t)W, plane);
}

// sum of three 64-bit counters over the workgroup; thread 0 gets it
__device__ inline void block_sum3(unsigned long long (&s)[3], unsigned long long (*red)[3])
{
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int o = 32; o; o >>= 1) s[q] += __shfl_xor(s[q], o);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < 3; ++q) red[threadIdx.x >> 6][q] = s[q];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            s[q] = red[0][q];
            for (int w = 1; w < YUV_THREADS / 64; ++w) s[q] += red[w][q];
        }
}

__device__ inline unsigned sqdiff(unsigned a, unsigned b)
{
    const unsigned d = a > b ? a - b : b - a;                   // 16-bit samples: d < 2^16, the square fits an unsigned 32-bit word
    return d * d;
}

// rgb: [B][3][H][W].  FLT: fp32 planes yf / uf / vf.  INT: integer planes yi / ui / vi; SSE (needs INT): source planes ys / us / vs and
// part[B][gridDim.x][3], the workgroup's sums of squared differences of Y, U, V.
template <typename T, bool VEC, bool FLT, bool INT, bool SSE>
__global__ __launch_bounds__(YUV_THREADS) void rgb_to_yuv420_kernel(const float *__restrict__ rgb, int H, int W, double peak,
                                                                    float *__restrict__ yf, float *__restrict__ uf, float *__restrict__ vf,
                                                                    T *__restrict__ yi, T *__restrict__ ui, T *__restrict__ vi,
                                                                    const T *__restrict__ ys, const T *__restrict__ us,
                                                                    const T *__restrict__ vs, unsigned long long *__restrict__ part)
{
    __shared__ unsigned long long red[YUV_THREADS / 64][3];
    const int Hc = H >> 1, Wc = W >> 1;
    const YuvItem it = yuv_item(Hc, W);
    const size_t b = blockIdx.y, plane = (size_t)H * W, cplane = (size_t)Hc * Wc;
    unsigned long long sse[3] = {0, 0, 0};

    if (it.live) {
        const int nc = it.valid >> 1;                           // chroma samples of this item: 2, or 1
        const size_t off = (size_t)(2 * it.cy) * W + it.x0;
        YuvItemOut<T> o;
        rgb_item_to_yuv420<T, VEC>(rgb + b * 3 * plane + off, (size_t)W, plane, it.valid, peak, o);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const size_t roff = b * plane + off + (size_t)r * W;
            if (FLT) store_n<VEC>(yf + roff, it.valid, o.yo[r]);
            if (INT) store_n<VEC>(yi + roff, it.valid, o.yq[r]);
            if (SSE) {
                T s[4];
                load_n<VEC>(ys + roff, it.valid, s);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < it.valid) sse[0] += sqdiff(o.yq[r][j], s[j]);
            }
        }
        const size_t coff = b * cplane + (size_t)it.cy * Wc + (it.x0 >> 1);
        if (FLT) {
            store_n<VEC>(uf + coff, nc, o.uo);
            store_n<VEC>(vf + coff, nc, o.vo);
        }
        if (INT) {
            store_n<VEC>(ui + coff, nc, o.uq);
            store_n<VEC>(vi + coff, nc, o.vq);
        }
        if (SSE) {
            T su[2], sv[2];
            load_n<VEC>(us + coff, nc, su);
            load_n<VEC>(vs + coff, nc, sv);
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (k < nc) sse[1] += sqdiff(o.uq[k], su[k]), sse[2] += sqdiff(o.vq[k], sv[k]);
        }
    }
    if (SSE) {
        block_sum3(sse, red);
        if (threadIdx.x == 0) {
            unsigned long long *dst = part + (b * gridDim.x + blockIdx.x) * 3;
            dst[0] = sse[0], dst[1] = sse[1], dst[2] = sse[2];
        }
    }
}

// one workgroup per image: sse[b][q] = sum over the image's nblk slots
__global__ __launch_bounds__(YUV_THREADS) void yuv_sse_final_kernel(const unsigned long long *__restrict__ part, int nblk,
                                                                    unsigned long long *__restrict__ sse)
{
    __shared__ unsigned long long red[YUV_THREADS / 64][3];
    const unsigned long long *src = part + (size_t)blockIdx.x * nblk * 3;
    unsigned long long s[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < nblk; i += YUV_THREADS) s[0] += src[3 * i], s[1] += src[3 * i + 1], s[2] += src[3 * i + 2];
    block_sum3(s, red);
    if (threadIdx.x == 0) {
        unsigned long long *dst = sse + (size_t)blockIdx.x * 3;
        dst[0] = s[0], dst[1] = s[1], dst[2] = s[2];
    }
}

// ---- the single steps on fp32 tensors (transforms.rgb2ycbcr / ycbcr2rgb / yuv_444_to_420 / yuv_420_to_444 on device tensors): fp32,
// the reference's order of operations.  Element-wise and plane-wise streaming kernels, one element per thread.
template <bool TO_RGB>
__global__ __launch_bounds__(YUV_THREADS) void ycbcr_convert_kernel(const float *__restrict__ in, float *__restrict__ out, size_t hw)
{
    const size_t i = (size_t)blockIdx.x * YUV_THREADS + threadIdx.x;
    if (i >= hw) return;
    const size_t base = (size_t)blockIdx.y * 3 * hw + i;
    const float a = in[base], b = in[base + hw], c = in[base + 2 * hw];
    const float kr = (float)KR, kg = (float)KG, kb = (float)KB;
    float o0, o1, o2;
    if (TO_RGB) {                                               // a, b, c = y, cb, cr
        o0 = a + (float)(2.0 - 2.0 * KR) * (c - 0.5f);
        o2 = a + (float)(2.0 - 2.0 * KB) * (b - 0.5f);
        o1 = (a - kr * o0 - kb * o2) / kg;
    } else {                                                    // a, b, c = r, g, b
        o0 = kr * a + kg * b + kb * c;
        o1 = 0.5f * (c - o0) / (float)(1.0 - KB) + 0.5f;
        o2 = 0.5f * (a - o0) / (float)(1.0 - KR) + 0.5f;
    }
    out[base] = o0, out[base + hw] = o1, out[base + 2 * hw] = o2;
}

// mode 0 / 1: [planes][H][W] -> [planes][2H][2W], bilinear (align_corners=False borders) / nearest; mode 2: -> [planes][H/2][W/2], 2 x 2 mean
__global__ __launch_bounds__(YUV_THREADS) void plane_resample2_kernel(const float *__restrict__ in, float *__restrict__ out, int H, int W, int mode)
{
    const int Ho = mode == 2 ? H >> 1 : H * 2, Wo = mode == 2 ? W >> 1 : W * 2;
    const size_t i = (size_t)blockIdx.x * YUV_THREADS + threadIdx.x;
    if (i >= (size_t)Ho * Wo) return;
    const int oy = (int)(i / Wo), ox = (int)(i - (size_t)oy * Wo);
    const float *p = in + (size_t)blockIdx.y * H * W;
    float r;
    if (mode == 2) {
        const float *q = p + (size_t)(2 * oy) * W + 2 * ox;
        r = (((q[0] + q[1]) + q[W]) + q[W + 1]) * 0.25f;
    } else if (mode == 1) {
        r = p[(size_t)(oy >> 1) * W + (ox >> 1)];
    } else {
        // source position (o + 0.5) / 2 - 0.5, clamped at 0: o = 0 -> sample 0 alone; odd o -> 0.75 / 0.25 of samples o/2, o/2 + 1;
        // even o -> 0.25 / 0.75 of samples o/2 - 1, o/2; the upper index clamped at the edge
        const int y0 = oy == 0 ? 0 : (oy - 1) >> 1, x0 = ox == 0 ? 0 : (ox - 1) >> 1;
        const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
        const float ly = oy == 0 ? 0.f : ((oy & 1) ? 0.25f : 0.75f), lx = ox == 0 ? 0.f : ((ox & 1) ? 0.25f : 0.75f);
        const float *r0 = p + (size_t)y0 * W, *r1 = p + (size_t)y1 * W;
        r = (1.f - ly) * ((1.f - lx) * r0[x0] + lx * r0[x1]) + ly * ((1.f - lx) * r1[x0] + lx * r1[x1]);
    }
    out[(size_t)blockIdx.y * Ho * Wo + i] = r;
}

template <typename T>
int launch_to_rgb(const void *y, const void *u, const void *v, int B, int H, int W, int nblk, float peak, int nearest, int clamp01, float *rgb,
                  hipStream_t st)
{
    const bool vec = W % 4 == 0 && aligned_to(y, 4 * sizeof(T)) && aligned_to(rgb, 16);
    const dim3 grid((unsigned)nblk, (unsigned)B), block(YUV_THREADS);
    const T *yp = static_cast<const T *>(y), *up = static_cast<const T *>(u), *vp = static_cast<const T *>(v);
    if (vec)
        hipLaunchKernelGGL((yuv420_to_rgb_kernel<T, true>), grid, block, 0, st, yp, up, vp, H, W, peak, nearest, clamp01, rgb);
    else
        hipLaunchKernelGGL((yuv420_to_rgb_kernel<T, false>), grid, block, 0, st, yp, up, vp, H, W, peak, nearest, clamp01, rgb);
    STEM_LAUNCH_CHECK("stem_yuv420_to_rgb");
    return 0;
}

template <typename T, bool VEC>
int launch_to_yuv(const float *rgb, int B, int H, int W, int nblk, double peak, float *yf, float *uf, float *vf, void *yi, void *ui, void *vi,
                  const void *ys, const void *us, const void *vs, unsigned long long *part, hipStream_t st)
{
    const dim3 grid((unsigned)nblk, (unsigned)B), block(YUV_THREADS);
    T *a = static_cast<T *>(yi), *b = static_cast<T *>(ui), *c = static_cast<T *>(vi);
    const T *d = static_cast<const T *>(ys), *e = static_cast<const T *>(us), *f = static_cast<const T *>(vs);
#define STEM_YUV_LAUNCH(FLT, INT, SSE) \
    hipLaunchKernelGGL((rgb_to_yuv420_kernel<T, VEC, FLT, INT, SSE>), grid, block, 0, st, rgb, H, W, peak, yf, uf, vf, a, b, c, d, e, f, part)
    if (yf && yi && ys)
        STEM_YUV_LAUNCH(true, true, true);
    else if (yf && yi)
        STEM_YUV_LAUNCH(true, true, false);
    else if (yf)
        STEM_YUV_LAUNCH(true, false, false);
    else if (ys)
        STEM_YUV_LAUNCH(false, true, true);
    else
        STEM_YUV_LAUNCH(false, true, false);
#undef STEM_YUV_LAUNCH
    STEM_LAUNCH_CHECK("stem_rgb_to_yuv420");
    return 0;
}

}   // namespace

STEM_EXPORT int stem_yuv420_to_rgb(const void *y, const void *u, const void *v, int B, int H, int W, int sample_bytes, int bit_depth,
                                   int upsample, int clamp01, float *rgb, void *stream)
{
    STEM_CHECK_ARG(y && u && v && rgb, "stem_yuv420_to_rgb: null pointer");
    int nblk;
    if (int rc = yuv_plan("stem_yuv420_to_rgb", B, H, W, sample_bytes, bit_depth, &nblk)) return rc;
    STEM_CHECK_ARG(upsample == STEM_YUV_BILINEAR || upsample == STEM_YUV_NEAREST, "stem_yuv420_to_rgb: upsample is 0 (bilinear) or 1 (nearest), got %d",
                   upsample);
    STEM_CHECK_ARG(aligned_to(y, sample_bytes) && aligned_to(u, sample_bytes) && aligned_to(v, sample_bytes) && aligned_to(rgb, 4),
                   "stem_yuv420_to_rgb: misaligned pointer");
    const float peak = (float)((1 << bit_depth) - 1);
    hipStream_t st = (hipStream_t)stream;
    if (sample_bytes == 1) return launch_to_rgb<uint8_t>(y, u, v, B, H, W, nblk, peak, upsample == STEM_YUV_NEAREST, clamp01 != 0, rgb, st);
    return launch_to_rgb<uint16_t>(y, u, v, B, H, W, nblk, peak, upsample == STEM_YUV_NEAREST, clamp01 != 0, rgb, st);
}

STEM_EXPORT int stem_rgb_to_yuv420_workspace(int B, int H, int W, size_t *bytes)
{
    STEM_CHECK_ARG(bytes, "stem_rgb_to_yuv420_workspace: null pointer");
    int nblk;
    if (int rc = yuv_plan("stem_rgb_to_yuv420_workspace", B, H, W, 1, 8, &nblk)) return rc;
    *bytes = (size_t)B * nblk * 3 * sizeof(unsigned long long);
    return 0;
}

STEM_EXPORT int stem_rgb_to_yuv420(const float *rgb, int B, int H, int W, float *yf, float *uf, float *vf, void *yi, void *ui, void *vi,
                                   int sample_bytes, int bit_depth, const void *ys, const void *us, const void *vs, void *workspace,
                                   size_t workspace_bytes, unsigned long long *sse, void *stream)
{
    STEM_CHECK_ARG(rgb, "stem_rgb_to_yuv420: null pointer (rgb)");
    const bool flt = yf || uf || vf, itg = yi || ui || vi, src = ys || us || vs;
    STEM_CHECK_ARG(flt || itg, "stem_rgb_to_yuv420: no output planes (null pointers)");
    STEM_CHECK_ARG(!flt || (yf && uf && vf), "stem_rgb_to_yuv420: null pointer among the fp32 planes");
    STEM_CHECK_ARG(!itg || (yi && ui && vi), "stem_rgb_to_yuv420: null pointer among the integer planes");
    STEM_CHECK_ARG(!src || (ys && us && vs && sse), "stem_rgb_to_yuv420: null pointer among the source planes and their sums");
    STEM_CHECK_ARG(!src || itg, "stem_rgb_to_yuv420: squared errors are taken against the integer planes, which are not asked for");
    STEM_CHECK_ARG(src || !sse, "stem_rgb_to_yuv420: sums asked for without source planes (null pointers)");
    int nblk;
    if (int rc = yuv_plan("stem_rgb_to_yuv420", B, H, W, itg ? sample_bytes : 1, itg ? bit_depth : 8, &nblk)) return rc;
    const size_t need = src ? (size_t)B * nblk * 3 * sizeof(unsigned long long) : 0;
    STEM_CHECK_ARG(!src || (workspace && workspace_bytes >= need), "stem_rgb_to_yuv420: workspace of %zu bytes, %zu needed (stem_rgb_to_yuv420_workspace)",
                   workspace ? workspace_bytes : (size_t)0, need);
    STEM_CHECK_ARG(aligned_to(workspace, 8) && aligned_to(sse, 8), "stem_rgb_to_yuv420: the workspace and the sums must be 8-byte aligned");
    const size_t sb = itg ? (size_t)sample_bytes : 1;
    STEM_CHECK_ARG(aligned_to(rgb, 4) && aligned_to(yf, 4) && aligned_to(uf, 4) && aligned_to(vf, 4) && aligned_to(yi, sb) && aligned_to(ui, sb) &&
                       aligned_to(vi, sb) && aligned_to(ys, sb) && aligned_to(us, sb) && aligned_to(vs, sb),
                   "stem_rgb_to_yuv420: misaligned pointer");

    const bool vec = W % 4 == 0 && aligned_to(rgb, 16) && aligned_to(yf, 16) && aligned_to(uf, 8) && aligned_to(vf, 8) && aligned_to(yi, 4 * sb) &&
                     aligned_to(ui, 2 * sb) && aligned_to(vi, 2 * sb) && aligned_to(ys, 4 * sb) && aligned_to(us, 2 * sb) && aligned_to(vs, 2 * sb);
    const double peak = (double)((1 << (itg ? bit_depth : 8)) - 1);
    unsigned long long *part = static_cast<unsigned long long *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (sb == 1)
        rc = vec ? launch_to_yuv<uint8_t, true>(rgb, B, H, W, nblk, peak, yf, uf, vf, yi, ui, vi, ys, us, vs, part, st)
                 : launch_to_yuv<uint8_t, false>(rgb, B, H, W, nblk, peak, yf, uf, vf, yi, ui, vi, ys, us, vs, part, st);
    else
        rc = vec ? launch_to_yuv<uint16_t, true>(rgb, B, H, W, nblk, peak, yf, uf, vf, yi, ui, vi, ys, us, vs, part, st)
                 : launch_to_yuv<uint16_t, false>(rgb, B, H, W, nblk, peak, yf, uf, vf, yi, ui, vi, ys, us, vs, part, st);
    if (rc) return rc;
    if (src) {
        hipLaunchKernelGGL(yuv_sse_final_kernel, dim3(B), dim3(YUV_THREADS), 0, st, part, nblk, sse);
        STEM_LAUNCH_CHECK("stem_rgb_to_yuv420");
    }
    return 0;
}

STEM_EXPORT int stem_ycbcr_convert(const float *in, float *out, int N, int H, int W, int to_rgb, void *stream)
{
    STEM_CHECK_ARG(in && out, "stem_ycbcr_convert: null pointer");
    STEM_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0, "stem_ycbcr_convert: [%d,3,%d,%d]: 1 .. 65535 images of positive size", N, H, W);
    const size_t hw = (size_t)H * W;
    const dim3 grid((unsigned)cdivz(hw, YUV_THREADS), (unsigned)N), block(YUV_THREADS);
    if (to_rgb)
        hipLaunchKernelGGL((ycbcr_convert_kernel<true>), grid, block, 0, (hipStream_t)stream, in, out, hw);
    else
        hipLaunchKernelGGL((ycbcr_convert_kernel<false>), grid, block, 0, (hipStream_t)stream, in, out, hw);
    STEM_LAUNCH_CHECK("stem_ycbcr_convert");
    return 0;
}

STEM_EXPORT int stem_plane_resample2(const float *in, float *out, int planes, int H, int W, int mode, void *stream)
{
    STEM_CHECK_ARG(in && out, "stem_plane_resample2: null pointer");
    STEM_CHECK_ARG(planes > 0 && planes <= 65535 && H > 0 && W > 0 && H < (1 << 30) && W < (1 << 30),
                   "stem_plane_resample2: %d planes of %d x %d: 1 .. 65535 planes of positive size", planes, H, W);
    STEM_CHECK_ARG(mode == STEM_YUV_BILINEAR || mode == STEM_YUV_NEAREST || mode == STEM_YUV_AVG_POOL, "stem_plane_resample2: mode is 0 (bilinear x2), 1 (nearest x2) or 2 (2 x 2 mean), got %d", mode);
    STEM_CHECK_ARG(mode != STEM_YUV_AVG_POOL || (H % 2 == 0 && W % 2 == 0), "stem_plane_resample2: the 2 x 2 mean needs even sides, got %d x %d", H, W);
    const size_t n = mode == STEM_YUV_AVG_POOL ? (size_t)(H / 2) * (W / 2) : (size_t)H * W * 4;
    const dim3 grid((unsigned)cdivz(n, YUV_THREADS), (unsigned)planes), block(YUV_THREADS);
    hipLaunchKernelGGL(plane_resample2_kernel, grid, block, 0, (hipStream_t)stream, in, out, H, W, mode);
    STEM_LAUNCH_CHECK("stem_plane_resample2");
    return 0;
}
