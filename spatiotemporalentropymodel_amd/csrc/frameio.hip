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

// blockIdx.x < nblk_img: image items; behind them: pad items (yuv_elem.h: pad_item_at).  pvec: a pad group of four aligned columns is one
// vector per plane.
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
    const PadItem pad = pad_item_at((long long)(blockIdx.x - nblk_img) * YUV_THREADS + threadIdx.x, Hp, Wp, top, left, H, W);
    if (!pad.live) return;
    zero_group(frame + (size_t)pad.row * Wp + pad.c0, oplane, pad.c1 - pad.c0, pvec && pad.c1 - pad.c0 == 4 && (pad.c0 & 3) == 0);
}

template <typename T, bool LVEC, bool SVEC>
__global__ __launch_bounds__(YUV_THREADS) void rgb_window_to_yuv420_kernel(const float *__restrict__ rgb, size_t row_pitch, size_t plane_pitch,
                                                                           int top, int left, int H, int W, double peak, T *__restrict__ yi,
                                                                           T *__restrict__ ui, T *__restrict__ vi)
{
    const YuvItem it = yuv_item_at((long long)blockIdx.x * YUV_THREADS + threadIdx.x, H >> 1, W);
    if (!it.live) return;
    const size_t b = blockIdx.y;
    rgb_window_item_to_planes<T, LVEC, SVEC>(rgb + b * 3 * plane_pitch, row_pitch, plane_pitch, top, left, H, W, b, it, peak, yi, ui, vi);
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
    const long long nblk_pad = (pad_item_count(Hp, Wp, left, H, W) + YUV_THREADS - 1) / YUV_THREADS;
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
