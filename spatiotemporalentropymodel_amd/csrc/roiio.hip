// The two per-frame device passes of the pixel-domain sequence codec (include/stem_roiio.h; libstem_roiio.so; video_pixel.py):
//     stem_rgb_window_recondition   bitstream.pad(bitstream.crop(x_hat)) in place + the window's integer 4:2:0 planes   one launch
//     stem_roi_map_padded           rectangles + a background level -> the zero-padded fp32 quality map                 one launch
//
// Recondition.  The reference conditions a P frame on the previous frame's CROPPED reconstruction, zero-padded again, so the border of
// the decoder's padded x_hat has to become zero before the frame is read as a condition.  The workgroups are those of frameio.hip's
// two kernels put behind each other, through the same functions of yuv_elem.h: first the image items of the emit kernel (2 rows x 4
// columns of luma each, rgb_window_item_to_planes: the planes are the emit kernel's bits; none when no planes are wanted), then the
// pad items of the ingest kernel (pad_item_at: the full rows above and below the window in groups of four columns, then the groups
// left and right of it), here over a pitched frame.
// In place is safe in ONE launch because every element of the frame is either read (window: image items only read it) or written
// (border: pad items only write it), never both: no item's result depends on another item's store, whatever order they run in.
// Elements between Wp and the row pitch belong to neither set.  HBM-bound: the window is read once (12 bytes per pixel) when planes
// are wanted, the border is written once.
//
// Rasteriser.  One work item is four columns of one row of the PADDED map, so the zero border and the window come out of one grid and
// every element is written exactly once (a poisoned output comes back clean).  The boxes are staged in LDS once per workgroup; the
// blend is written with plain operators under `#pragma clang fp contract(off)`, so that each of the subtraction, the product and the
// sum rounds to fp32 as tests/roi_map_ref.py does with numpy (the __f*_rn functions are plain operators in a header that is compiled
// with contraction on: a product and a sum stated through them still fuse into one FMA after inlining, so they are not used here).
// The distance to the box's edge is taken in unsigned arithmetic: inside a box all
// four differences are non-negative and below 2^32 whatever the box's corners are, so nothing overflows.
#include <stdarg.h>

#include "../../include/stem_roiio.h"
#include "stem_common.h"
#include "yuv_elem.h"

#pragma clang fp contract(off)

// this library's own message slot
static thread_local char g_err[512] = "";
void stem_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
STEM_EXPORT const char *stem_roiio_last_error(void) { return g_err; }

namespace {

using namespace yuv_elem;

// blockIdx.x < nblk_img: image items (they READ the window and write the planes); behind them: pad items (they WRITE the border).
// pvec: a pad group of four aligned columns is one vector per plane.  rgb carries no __restrict__: both kinds of item go through it.
template <typename T, bool LVEC, bool SVEC>
__global__ __launch_bounds__(YUV_THREADS) void rgb_window_recondition_kernel(float *rgb, int Hp, int Wp, size_t row_pitch, size_t plane_pitch, int top,
                                                                             int left, int H, int W, double peak, T *__restrict__ yi,
                                                                             T *__restrict__ ui, T *__restrict__ vi, int nblk_img, int pvec)
{
    const size_t b = blockIdx.y;
    float *frame = rgb + b * 3 * plane_pitch;
    if ((int)blockIdx.x < nblk_img) {
        const YuvItem it = yuv_item_at((long long)blockIdx.x * YUV_THREADS + threadIdx.x, H >> 1, W);
        if (it.live) rgb_window_item_to_planes<T, LVEC, SVEC>(frame, row_pitch, plane_pitch, top, left, H, W, b, it, peak, yi, ui, vi);
        return;
    }
    const PadItem pad = pad_item_at((long long)(blockIdx.x - nblk_img) * YUV_THREADS + threadIdx.x, Hp, Wp, top, left, H, W);
    if (!pad.live) return;
    zero_group(frame + (size_t)pad.row * row_pitch + pad.c0, plane_pitch, pad.c1 - pad.c0, pvec && pad.c1 - pad.c0 == 4 && (pad.c0 & 3) == 0);
}

constexpr int ROI_THREADS = 256;

// one item: columns 4 g .. 4 g + 4 of row `row` of the padded map
template <bool VEC>
__global__ __launch_bounds__(ROI_THREADS) void roi_map_padded_kernel(const int32_t *__restrict__ boxes, const float *__restrict__ values, int n,
                                                                     float background, float *__restrict__ map, int Hp, int Wp, int top, int left,
                                                                     int H, int W)
{
    __shared__ int32_t sbox[STEM_ROI_MAX_BOXES][5];
    __shared__ float sval[STEM_ROI_MAX_BOXES];
    for (int i = threadIdx.x; i < n * 5; i += ROI_THREADS) sbox[i / 5][i % 5] = boxes[i];
    for (int i = threadIdx.x; i < n; i += ROI_THREADS) sval[i] = values[i];
    __syncthreads();
    const int gW = (Wp + 3) >> 2;
    const long long p = (long long)blockIdx.x * ROI_THREADS + threadIdx.x;
    if (p >= (long long)Hp * gW) return;
    const int row = (int)(p / gW), c0 = (int)(p - (long long)row * gW) * 4;
    const int valid = Wp - c0 < 4 ? Wp - c0 : 4;
    const int r = row - top;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r >= 0 && r < H && c0 + 4 > left && c0 < left + W) {
        bool in[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j - left;
            in[j] = c >= 0 && c < W;
            if (in[j]) v[j] = background;
        }
        for (int k = 0; k < n; ++k) {
            const int x0 = sbox[k][0], y0 = sbox[k][1], x1 = sbox[k][2], y1 = sbox[k][3], feather = sbox[k][4];
            if (r < y0 || r >= y1) continue;
            const unsigned dy0 = (unsigned)r - (unsigned)y0, dy1 = (unsigned)y1 - 1u - (unsigned)r;
            const unsigned dy = dy0 < dy1 ? dy0 : dy1;
            const float val = sval[k], fden = (float)((unsigned)feather + 1u);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j - left;
                if (!in[j] || c < x0 || c >= x1) continue;
                const unsigned dx0 = (unsigned)c - (unsigned)x0, dx1 = (unsigned)x1 - 1u - (unsigned)c;
                const unsigned dx = dx0 < dx1 ? dx0 : dx1, d = dx < dy ? dx : dy;
                if (d >= (unsigned)feather) {
                    v[j] = val;
                } else {
                    const float t = (float)(d + 1u) / fden;     // correctly rounded: hipcc's default for fp32 division
                    const float diff = val - v[j];
                    const float prod = diff * t;                // no FMA with the sum below: contraction is off in this file
                    v[j] = v[j] + prod;
                }
            }
        }
    }
    store_n<VEC>(map + (size_t)row * Wp + c0, valid, v);
}

template <typename T>
int launch_recondition(float *rgb, int B, int Hp, int Wp, size_t row_pitch, size_t plane_pitch, int top, int left, int H, int W, int nblk_img,
                       int nblk_pad, double peak, void *yi, void *ui, void *vi, hipStream_t st)
{
    const bool pvec = row_pitch % 4 == 0 && plane_pitch % 4 == 0 && aligned_to(rgb, 16);
    const bool lvec = pvec && W % 4 == 0 && left % 4 == 0;
    const bool svec = W % 4 == 0 && aligned_to(yi, 4 * sizeof(T)) && aligned_to(ui, 2 * sizeof(T)) && aligned_to(vi, 2 * sizeof(T));
    const dim3 grid((unsigned)(nblk_img + nblk_pad), (unsigned)B), block(YUV_THREADS);
    T *a = static_cast<T *>(yi), *b = static_cast<T *>(ui), *c = static_cast<T *>(vi);
#define STEM_RECOND_LAUNCH(L, S)                                                                                                                \
    hipLaunchKernelGGL((rgb_window_recondition_kernel<T, L, S>), grid, block, 0, st, rgb, Hp, Wp, row_pitch, plane_pitch, top, left, H, W, peak, a, b, \
                       c, nblk_img, (int)pvec)
    if (lvec && svec)
        STEM_RECOND_LAUNCH(true, true);
    else if (lvec)
        STEM_RECOND_LAUNCH(true, false);
    else if (svec)
        STEM_RECOND_LAUNCH(false, true);
    else
        STEM_RECOND_LAUNCH(false, false);
#undef STEM_RECOND_LAUNCH
    STEM_LAUNCH_CHECK("stem_rgb_window_recondition");
    return 0;
}

}   // namespace

STEM_EXPORT int stem_rgb_window_recondition(float *rgb, int B, int Hp, int Wp, size_t row_pitch, size_t plane_pitch, int top, int left, int H, int W,
                                            void *yi, void *ui, void *vi, int sample_bytes, int bit_depth, void *stream)
{
    const char *who = "stem_rgb_window_recondition";
    STEM_CHECK_ARG(rgb, "%s: null pointer", who);
    const int planes = (yi != nullptr) + (ui != nullptr) + (vi != nullptr);
    STEM_CHECK_ARG(planes == 0 || planes == 3, "%s: the three plane pointers are all given or all NULL, got %d of them", who, planes);
    int nblk_img;
    if (int rc = yuv_plan(who, B, H, W, sample_bytes, bit_depth, &nblk_img)) return rc;
    if (int rc = window_fits(who, Hp, Wp, top, left, H, W)) return rc;
    STEM_CHECK_ARG(row_pitch >= (size_t)Wp && row_pitch < ((size_t)1 << 40), "%s: a row pitch of %zu floats for rows of %d", who, row_pitch, Wp);
    STEM_CHECK_ARG(plane_pitch >= (size_t)(Hp - 1) * row_pitch + (size_t)Wp && plane_pitch < ((size_t)1 << 50),
                   "%s: a plane pitch of %zu floats for %d rows %zu apart", who, plane_pitch, Hp, row_pitch);
    const size_t sb = (size_t)sample_bytes;
    STEM_CHECK_ARG(aligned_to(rgb, 4) && aligned_to(yi, sb) && aligned_to(ui, sb) && aligned_to(vi, sb), "%s: misaligned pointer", who);
    if (!planes) nblk_img = 0;
    const long long nblk_pad = (pad_item_count(Hp, Wp, left, H, W) + YUV_THREADS - 1) / YUV_THREADS;
    STEM_CHECK_ARG(nblk_img + nblk_pad <= 0x7fffffffLL, "%s: a frame of %d x %d is too large", who, Hp, Wp);
    if (nblk_img + nblk_pad == 0) return 0;                     // no border and no planes: nothing to do
    const double peak = (double)((1 << bit_depth) - 1);
    hipStream_t st = (hipStream_t)stream;
    if (sb == 1) return launch_recondition<uint8_t>(rgb, B, Hp, Wp, row_pitch, plane_pitch, top, left, H, W, nblk_img, (int)nblk_pad, peak, yi, ui, vi, st);
    return launch_recondition<uint16_t>(rgb, B, Hp, Wp, row_pitch, plane_pitch, top, left, H, W, nblk_img, (int)nblk_pad, peak, yi, ui, vi, st);
}

STEM_EXPORT int stem_roi_map_padded(const int32_t *boxes, const float *values, int n, float background, float *map, int Hp, int Wp, int top, int left,
                                    int H, int W, void *stream)
{
    const char *who = "stem_roi_map_padded";
    STEM_CHECK_ARG(map, "%s: null pointer", who);
    STEM_CHECK_ARG(n >= 0 && n <= STEM_ROI_MAX_BOXES, "%s: 0 .. %d boxes, got %d", who, STEM_ROI_MAX_BOXES, n);
    STEM_CHECK_ARG(n == 0 || (boxes && values), "%s: null pointer (%d boxes need both arrays)", who, n);
    STEM_CHECK_ARG(H >= 1 && W >= 1, "%s: a window of %d x %d", who, H, W);
    if (int rc = window_fits(who, Hp, Wp, top, left, H, W)) return rc;
    STEM_CHECK_ARG(aligned_to(boxes, 4) && aligned_to(values, 4) && aligned_to(map, 4), "%s: misaligned pointer", who);
    const long long items = (long long)Hp * ((Wp + 3) / 4);
    const long long nblk = (items + ROI_THREADS - 1) / ROI_THREADS;
    STEM_CHECK_ARG(nblk <= 0x7fffffffLL, "%s: a frame of %d x %d is too large", who, Hp, Wp);
    const dim3 grid((unsigned)nblk), block(ROI_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (Wp % 4 == 0 && aligned_to(map, 16))
        hipLaunchKernelGGL((roi_map_padded_kernel<true>), grid, block, 0, st, boxes, values, n, background, map, Hp, Wp, top, left, H, W);
    else
        hipLaunchKernelGGL((roi_map_padded_kernel<false>), grid, block, 0, st, boxes, values, n, background, map, Hp, Wp, top, left, H, W);
    STEM_LAUNCH_CHECK("stem_roi_map_padded");
    return 0;
}
