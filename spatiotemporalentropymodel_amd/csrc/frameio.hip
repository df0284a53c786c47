// Frame ingest and emit of the stand-alone sequence codec (include/stem_frameio.h; libstem_frameio.so):
//     stem_yuv420_to_rgb_padded    bitstream.pad(stem_yuv420_to_rgb(planes))              one launch, the pad written as +0.0
//     stem_rgb_window_to_yuv420    stem_rgb_to_yuv420(bitstream.crop(frame)) -> integers  one launch, reads the window in place
// The work items and their arithmetic are yuv.hip's (yuv_elem.h: 2 rows x 4 columns of luma in IMAGE coordinates), so the bits are
// too; what differs is where an item's pixels sit -- at (top, left) of a frame with its own row and plane pitches -- and which of
// its accesses may be vectors.  Loads and stores are judged separately: the dense side of either kernel (the integer planes) is a
// vector whenever W % 4 == 0, the padded side only when left, the row pitch and the plane pitch are multiples of four as well (1080p
// in 1088 x 1920: top 4, left 0).  An odd offset runs the same body element by element.
//
// Ingest also owns the pad.  The workgroups behind the image's are numbered over the pad alone: first the Hp - H full rows above and
// below the image in groups of four columns, then, row by row of the image, the groups left and right of it (the right ones start
// at left + W, whatever its alignment).  No element is written twice and none is skipped, so a poisoned output comes back clean.
// Both are HBM-bound passes: 12 bytes per pixel on the fp32 side, 1.5 or 3 on the integer side.
#include <stdarg.h>

#include "../../include/stem_frameio.h"
#include "stem_common.h"
#include "yuv_elem.h"

// this library's own message slot (libstem_hip.so keeps its own behind stem_last_error)
static thread_local char g_err[512] = "";
void stem_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
STEM_EXPORT const char *stem_frameio_last_error(void) { return g_err; }

namespace {

using namespace yuv_elem;

// four (or fewer) zeros into each colour plane at o
__device__ inline void zero_group(float *o, size_t plane, int n, bool vec)
{
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        store_n<true>(o, 4, z), store_n<true>(o + plane, 4, z), store_n<true>(o + 2 * plane, 4, z);
    } else {
        store_n<false>(o, n, z), store_n<false>(o + plane, n, z), store_n<false>(o + 2 * plane, n, z);
    }
}

// blockIdx.x < nblk_img: image items; behind them: pad items.  pvec: a pad group of four aligned columns is one vector per plane.
template <typename T, bool LVEC, bool SVEC>
__global__ __launch_bounds__(YUV_THREADS) void yuv420_to_rgb_padded_kernel(const T *__restrict__ yp, const T *__restrict__ up,
                                                                           const T *__restrict__ vp, int H, int W, float peak, int nearest,
                                                                           int clamp01, float *__restrict__ rgb, int Hp, int Wp, int top,
                                                                           int left, int nblk_img, int pvec)
{
    const int Hc = H >> 1, Wc = W >> 1;
    const size_t b = blockIdx.y, oplane = (size_t)Hp * Wp;
    float *frame = rgb + b * 3 * oplane;
    if ((int)blockIdx.x < nblk_img) {
        const YuvItem it = yuv_item_at((long long)blockIdx.x * YUV_THREADS + threadIdx.x, Hc, W);
        if (!it.live) return;
        const size_t plane = (size_t)H * W, cplane = (size_t)Hc * Wc;
        yuv420_item_to_rgb<T, LVEC, SVEC>(yp + b * plane, up + b * cplane, vp + b * cplane, H, W, it, peak, nearest, clamp01,
                                          frame + (size_t)top * Wp + left, (size_t)Wp, oplane);
        return;
    }
    long long p = (long long)(blockIdx.x - nblk_img) * YUV_THREADS + threadIdx.x;
    const int gW = (Wp + 3) >> 2;
    const long long bands = (long long)(Hp - H) * gW;
    int row, c0, c1;
    if (p < bands) {                                            // the full rows above and below the image
        const int r = (int)(p / gW);
        row = r < top ? r : r + H;
        c0 = (int)(p - (long long)r * gW) * 4;
        c1 = c0 + 4 < Wp ? c0 + 4 : Wp;
    } else {                                                    // left and right of the image
        p -= bands;
        const int right0 = left + W, gL = (left + 3) >> 2, gR = (Wp - right0 + 3) >> 2, gs = gL + gR;
        if (gs == 0 || p >= (long long)H * gs) return;
        const int r = (int)(p / gs), g = (int)(p - (long long)r * gs);
        row = top + r;
        if (g < gL) {
            c0 = 4 * g;
            c1 = c0 + 4 < left ? c0 + 4 : left;
        } else {
            c0 = right0 + 4 * (g - gL);
            c1 = c0 + 4 < Wp ? c0 + 4 : Wp;
        }
    }
    zero_group(frame + (size_t)row * Wp + c0, oplane, c1 - c0, pvec && c1 - c0 == 4 && (c0 & 3) == 0);
}

template <typename T, bool LVEC, bool SVEC>
__global__ __launch_bounds__(YUV_THREADS) void rgb_window_to_yuv420_kernel(const float *__restrict__ rgb, size_t row_pitch, size_t plane_pitch,
                                                                           int top, int left, int H, int W, double peak, T *__restrict__ yi,
                                                                           T *__restrict__ ui, T *__restrict__ vi)
{
    const int Hc = H >> 1, Wc = W >> 1;
    const YuvItem it = yuv_item_at((long long)blockIdx.x * YUV_THREADS + threadIdx.x, Hc, W);
    if (!it.live) return;
    const size_t b = blockIdx.y, plane = (size_t)H * W, cplane = (size_t)Hc * Wc;
    const int nc = it.valid >> 1;                               // chroma samples of this item: 2, or 1
    YuvItemOut<T> o;
    rgb_item_to_yuv420<T, LVEC>(rgb + b * 3 * plane_pitch + (size_t)(top + 2 * it.cy) * row_pitch + left + it.x0, row_pitch, plane_pitch, it.valid,
                                peak, o);
    const size_t off = b * plane + (size_t)(2 * it.cy) * W + it.x0;
    store_n<SVEC>(yi + off, it.valid, o.yq[0]);
    store_n<SVEC>(yi + off + W, it.valid, o.yq[1]);
    const size_t coff = b * cplane + (size_t)it.cy * Wc + (it.x0 >> 1);
    store_n<SVEC>(ui + coff, nc, o.uq);
    store_n<SVEC>(vi + coff, nc, o.vq);
}

// the window of H x W at (top, left) lies inside Hp x Wp
int window_fits(const char *who, int Hp, int Wp, int top, int left, int H, int W)
{
    STEM_CHECK_ARG(Hp > 0 && Wp > 0 && Hp < (1 << 30) && Wp < (1 << 30), "%s: a frame of %d x %d", who, Hp, Wp);
    STEM_CHECK_ARG(top >= 0 && left >= 0 && top <= Hp - H && left <= Wp - W, "%s: the %d x %d window at (%d, %d) does not fit a frame of %d x %d", who, H,
                   W, top, left, Hp, Wp);
    return 0;
}

template <typename T>
int launch_ingest(const void *y, const void *u, const void *v, int B, int H, int W, int nblk_img, int nblk_pad, float peak, int nearest, int clamp01,
                  float *rgb, int Hp, int Wp, int top, int left, hipStream_t st)
{
    const bool lvec = W % 4 == 0 && aligned_to(y, 4 * sizeof(T));
    const bool pvec = Wp % 4 == 0 && aligned_to(rgb, 16);
    const bool svec = pvec && W % 4 == 0 && left % 4 == 0;
    const dim3 grid((unsigned)(nblk_img + nblk_pad), (unsigned)B), block(YUV_THREADS);
    const T *yp = static_cast<const T *>(y), *up = static_cast<const T *>(u), *vp = static_cast<const T *>(v);
#define STEM_INGEST_LAUNCH(L, S)                                                                                                         \
    hipLaunchKernelGGL((yuv420_to_rgb_padded_kernel<T, L, S>), grid, block, 0, st, yp, up, vp, H, W, peak, nearest, clamp01, rgb, Hp, Wp, top, \
                       left, nblk_img, (int)pvec)
    if (lvec && svec)
        STEM_INGEST_LAUNCH(true, true);
    else if (lvec)
        STEM_INGEST_LAUNCH(true, false);
    else if (svec)
        STEM_INGEST_LAUNCH(false, true);
    else
        STEM_INGEST_LAUNCH(false, false);
#undef STEM_INGEST_LAUNCH
    STEM_LAUNCH_CHECK("stem_yuv420_to_rgb_padded");
    return 0;
}

template <typename T>
int launch_emit(const float *rgb, int B, size_t row_pitch, size_t plane_pitch, int top, int left, int H, int W, int nblk, double peak, void *yi,
                void *ui, void *vi, hipStream_t st)
{
    const bool lvec = W % 4 == 0 && left % 4 == 0 && row_pitch % 4 == 0 && plane_pitch % 4 == 0 && aligned_to(rgb, 16);
    const bool svec = W % 4 == 0 && aligned_to(yi, 4 * sizeof(T)) && aligned_to(ui, 2 * sizeof(T)) && aligned_to(vi, 2 * sizeof(T));
    const dim3 grid((unsigned)nblk, (unsigned)B), block(YUV_THREADS);
    T *a = static_cast<T *>(yi), *b = static_cast<T *>(ui), *c = static_cast<T *>(vi);
#define STEM_EMIT_LAUNCH(L, S) \
    hipLaunchKernelGGL((rgb_window_to_yuv420_kernel<T, L, S>), grid, block, 0, st, rgb, row_pitch, plane_pitch, top, left, H, W, peak, a, b, c)
    if (lvec && svec)
        STEM_EMIT_LAUNCH(true, true);
    else if (lvec)
        STEM_EMIT_LAUNCH(true, false);
    else if (svec)
        STEM_EMIT_LAUNCH(false, true);
    else
        STEM_EMIT_LAUNCH(false, false);
#undef STEM_EMIT_LAUNCH
    STEM_LAUNCH_CHECK("stem_rgb_window_to_yuv420");
    return 0;
}

}   // namespace

STEM_EXPORT int stem_yuv420_to_rgb_padded(const void *y, const void *u, const void *v, int B, int H, int W, int sample_bytes, int bit_depth,
                                          int upsample, int clamp01, float *rgb, int Hp, int Wp, int top, int left, void *stream)
{
    const char *who = "stem_yuv420_to_rgb_padded";
    STEM_CHECK_ARG(y && u && v && rgb, "%s: null pointer", who);
    int nblk_img;
    if (int rc = yuv_plan(who, B, H, W, sample_bytes, bit_depth, &nblk_img)) return rc;
    STEM_CHECK_ARG(upsample == STEM_YUV_BILINEAR || upsample == STEM_YUV_NEAREST, "%s: upsample is 0 (bilinear) or 1 (nearest), got %d", who, upsample);
    if (int rc = window_fits(who, Hp, Wp, top, left, H, W)) return rc;
    STEM_CHECK_ARG(aligned_to(y, sample_bytes) && aligned_to(u, sample_bytes) && aligned_to(v, sample_bytes) && aligned_to(rgb, 4),
                   "%s: misaligned pointer", who);
    // pad items: the full rows, then the groups beside the image (yuv420_to_rgb_padded_kernel numbers them the same way)
    const long long pad_items = (long long)(Hp - H) * ((Wp + 3) / 4) + (long long)H * ((left + 3) / 4 + (Wp - left - W + 3) / 4);
    const long long nblk_pad = (pad_items + YUV_THREADS - 1) / YUV_THREADS;
    STEM_CHECK_ARG(nblk_img + nblk_pad <= 0x7fffffffLL, "%s: a frame of %d x %d is too large", who, Hp, Wp);
    const float peak = (float)((1 << bit_depth) - 1);
    hipStream_t st = (hipStream_t)stream;
    if (sample_bytes == 1)
        return launch_ingest<uint8_t>(y, u, v, B, H, W, nblk_img, (int)nblk_pad, peak, upsample == STEM_YUV_NEAREST, clamp01 != 0, rgb, Hp, Wp, top, left, st);
    return launch_ingest<uint16_t>(y, u, v, B, H, W, nblk_img, (int)nblk_pad, peak, upsample == STEM_YUV_NEAREST, clamp01 != 0, rgb, Hp, Wp, top, left, st);
}

STEM_EXPORT int stem_rgb_window_to_yuv420(const float *rgb, int B, int Hp, int Wp, size_t row_pitch, size_t plane_pitch, int top, int left, int H,
                                          int W, void *yi, void *ui, void *vi, int sample_bytes, int bit_depth, void *stream)
{
    const char *who = "stem_rgb_window_to_yuv420";
    STEM_CHECK_ARG(rgb && yi && ui && vi, "%s: null pointer", who);
    int nblk;
    if (int rc = yuv_plan(who, B, H, W, sample_bytes, bit_depth, &nblk)) return rc;
    if (int rc = window_fits(who, Hp, Wp, top, left, H, W)) return rc;
    STEM_CHECK_ARG(row_pitch >= (size_t)Wp && row_pitch < ((size_t)1 << 40), "%s: a row pitch of %zu floats for rows of %d", who, row_pitch, Wp);
    STEM_CHECK_ARG(plane_pitch >= (size_t)(Hp - 1) * row_pitch + (size_t)Wp && plane_pitch < ((size_t)1 << 50),
                   "%s: a plane pitch of %zu floats for %d rows %zu apart", who, plane_pitch, Hp, row_pitch);
    const size_t sb = (size_t)sample_bytes;
    STEM_CHECK_ARG(aligned_to(rgb, 4) && aligned_to(yi, sb) && aligned_to(ui, sb) && aligned_to(vi, sb), "%s: misaligned pointer", who);
    const double peak = (double)((1 << bit_depth) - 1);
    hipStream_t st = (hipStream_t)stream;
    if (sb == 1) return launch_emit<uint8_t>(rgb, B, row_pitch, plane_pitch, top, left, H, W, nblk, peak, yi, ui, vi, st);
    return launch_emit<uint16_t>(rgb, B, row_pitch, plane_pitch, top, left, H, W, nblk, peak, yi, ui, vi, st);
}
