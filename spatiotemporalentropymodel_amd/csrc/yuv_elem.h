// The arithmetic of the raw-frame kernels, stated once: yuv.hip (dense frames: stem_yuv420_to_rgb, stem_rgb_to_yuv420) and frameio.hip
// (a frame inside a padded one: stem_yuv420_to_rgb_padded, stem_rgb_window_to_yuv420) include this file and differ only in where a
// work item's samples live -- row and plane pitches, and which accesses may be vectors; roiio.hip (stem_rgb_window_recondition) takes
// the emit kernel's image item and the ingest kernel's pad items from here as well.  A work item is 2 rows x 4 columns of luma
// = 1 row x 2 columns of chroma, in IMAGE coordinates: the chroma taps clamp at the image's edge whatever surrounds the image in
// memory, and the 2 x 2 chroma blocks are aligned to the image.  The orders of operations are those yuv.hip documents; the integer
// planes and fp32 pixels of the two files are the same bits because they come out of these functions.
#pragma once
#include "stem_common.h"

namespace yuv_elem {

constexpr int YUV_THREADS = 256;
constexpr double KR = 0.2126, KG = 0.7152, KB = 0.0722;           // ITU-R BT.709 (functional.py:8-11)

template <typename T, int N>
struct alignas(sizeof(T) * N) Pack {
    T v[N];
};

// N consecutive samples; VEC: one aligned vector access (the caller guarantees alignment and that all N exist)
template <bool VEC, typename T, int N>
__device__ inline void load_n(const T *p, int valid, T (&out)[N])
{
    if (VEC) {
        const Pack<T, N> q = *reinterpret_cast<const Pack<T, N> *>(p);
#pragma unroll
        for (int i = 0; i < N; ++i) out[i] = q.v[i];
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) out[i] = i < valid ? p[i] : T(0);
    }
}
template <bool VEC, typename T, int N>
__device__ inline void store_n(T *p, int valid, const T (&in)[N])
{
    if (VEC) {
        Pack<T, N> q;
#pragma unroll
        for (int i = 0; i < N; ++i) q.v[i] = in[i];
        *reinterpret_cast<Pack<T, N> *>(p) = q;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (i < valid) p[i] = in[i];
    }
}

// work item t of an image with Hc chroma rows and W luma columns: chroma row cy, luma columns x0 .. x0 + 4 (the first `valid` exist)
struct YuvItem {
    int cy, x0, valid;
    bool live;
};
__device__ inline YuvItem yuv_item_at(long long t, int Hc, int W)
{
    const int wq = (W + 3) >> 2;
    YuvItem it;
    it.live = t < (long long)Hc * wq;
    it.cy = (int)(t / wq);
    it.x0 = (int)(t - (long long)it.cy * wq) * 4;
    it.valid = W - it.x0 < 4 ? W - it.x0 : 4;                   // 4, or 2 in the last item of a row with W % 4 == 2
    return it;
}

// ---- yuv -> rgb ------------------------------------------------------------------------------------------------------------------
// One item of one image.  yp / up / vp: the image's planes (dense, H x W and Hc x Wc).  out: where the image's pixel (0, 0) of the R
// plane goes; rows are out_row floats apart, the colour planes out_plane.  LVEC: the luma of an item is one aligned vector; SVEC: so
// are its four floats of each colour row.
template <typename T, bool LVEC, bool SVEC>
__device__ inline void yuv420_item_to_rgb(const T *__restrict__ yp, const T *__restrict__ up, const T *__restrict__ vp, int H, int W,
                                          const YuvItem it, float peak, int nearest, int clamp01, float *__restrict__ out, size_t out_row,
                                          size_t out_plane)
{
    const int Hc = H >> 1, Wc = W >> 1;
    const int cy = it.cy, k0 = it.x0 >> 1;

    // chroma of the item's 2 x 4 pixels, still in sample units: c[plane][row][column]
    float c[2][2][4];
    const T *cp[2] = {up, vp};
    if (nearest) {
        const int k1 = k0 + 1 < Wc ? k0 + 1 : Wc - 1;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float a = (float)cp[p][(size_t)cy * Wc + k0], d = (float)cp[p][(size_t)cy * Wc + k1];
#pragma unroll
            for (int r = 0; r < 2; ++r) c[p][r][0] = c[p][r][1] = a, c[p][r][2] = c[p][r][3] = d;
        }
    } else {
        // rows cy - 1, cy, cy + 1 and columns k0 - 1 .. k0 + 2, clamped into the plane
        const int rr[3] = {cy > 0 ? cy - 1 : 0, cy, cy + 1 < Hc ? cy + 1 : Hc - 1};
        int cc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 - 1 + j;
            cc[j] = k < 0 ? 0 : (k < Wc ? k : Wc - 1);
        }
        // torch's source index of output 0 is sample 0 with weight 1 (not 0.25 / 0.75 of the same sample twice: that sum rounds)
        const float wl0 = k0 == 0 ? 1.f : 0.25f, wl1 = k0 == 0 ? 0.f : 0.75f;
        const float wt0 = cy == 0 ? 1.f : 0.25f, wt1 = cy == 0 ? 0.f : 0.75f;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float h[3][4];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const T *row = cp[p] + (size_t)rr[r] * Wc;
                const float s0 = (float)row[cc[0]], s1 = (float)row[cc[1]], s2 = (float)row[cc[2]], s3 = (float)row[cc[3]];
                h[r][0] = wl0 * s0 + wl1 * s1;
                h[r][1] = 0.75f * s1 + 0.25f * s2;
                h[r][2] = 0.25f * s1 + 0.75f * s2;
                h[r][3] = 0.75f * s2 + 0.25f * s3;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[p][0][j] = wt0 * h[0][j] + wt1 * h[1][j];
                c[p][1][j] = 0.75f * h[1][j] + 0.25f * h[2][j];
            }
        }
    }

    const float c_r = (float)(2.0 - 2.0 * KR), c_b = (float)(2.0 - 2.0 * KB), kr = (float)KR, kg = (float)KG, kb = (float)KB;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        T ys[4];
        load_n<LVEC>(yp + (size_t)(2 * cy + r) * W + it.x0, it.valid, ys);
        float R[4], G[4], B[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = (float)ys[j] / peak, cb = c[0][r][j] / peak, cr = c[1][r][j] / peak;
            float rv = y + c_r * (cr - 0.5f);
            float bv = y + c_b * (cb - 0.5f);
            float gv = (y - kr * rv - kb * bv) / kg;
            if (clamp01) {
                rv = fminf(fmaxf(rv, 0.f), 1.f);
                gv = fminf(fmaxf(gv, 0.f), 1.f);
                bv = fminf(fmaxf(bv, 0.f), 1.f);
            }
            R[j] = rv, G[j] = gv, B[j] = bv;
        }
        float *o = out + (size_t)(2 * cy + r) * out_row + it.x0;
        store_n<SVEC>(o, it.valid, R);
        store_n<SVEC>(o + out_plane, it.valid, G);
        store_n<SVEC>(o + 2 * out_plane, it.valid, B);
    }
}

// ---- rgb -> yuv ------------------------------------------------------------------------------------------------------------------
// What one item becomes: its 2 x 4 luma and 1 x 2 chroma values, as fp32 (the fp64 value rounded once) and as integer samples
// rint(clamp(value, 0, 1) * peak), half to even.
template <typename T>
struct YuvItemOut {
    float yo[2][4], uo[2], vo[2];
    T yq[2][4], uq[2], vq[2];
};

// src: the item's first R value (image row 2 cy, column x0); rows src_row floats apart, colour planes src_plane.  fp64 arithmetic.
template <typename T, bool LVEC>
__device__ inline void rgb_item_to_yuv420(const float *__restrict__ src, size_t src_row, size_t src_plane, int valid, double peak,
                                          YuvItemOut<T> &o)
{
    double du[2] = {0.0, 0.0}, dv[2] = {0.0, 0.0};              // sums of b - y and r - y over each 2 x 2 block
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float *s = src + (size_t)r * src_row;
        float R[4], G[4], B[4];
        load_n<LVEC>(s, valid, R);
        load_n<LVEC>(s + src_plane, valid, G);
        load_n<LVEC>(s + 2 * src_plane, valid, B);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double rv = (double)R[j], gv = (double)G[j], bv = (double)B[j];
            const double y = KR * rv + KG * gv + KB * bv;
            du[j >> 1] += bv - y;
            dv[j >> 1] += rv - y;
            o.yo[r][j] = (float)y;
            o.yq[r][j] = (T)rint(fmin(fmax(y, 0.0), 1.0) * peak);
        }
    }
    // cb = 0.5 * (b - y) / (1 - Kb) + 0.5 averaged over the block (:41-42, :90): the average commutes with the affine map
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double cb = (0.25 * du[k]) * (0.5 / (1.0 - KB)) + 0.5, cr = (0.25 * dv[k]) * (0.5 / (1.0 - KR)) + 0.5;
        o.uo[k] = (float)cb, o.vo[k] = (float)cr;
        o.uq[k] = (T)rint(fmin(fmax(cb, 0.0), 1.0) * peak);
        o.vq[k] = (T)rint(fmin(fmax(cr, 0.0), 1.0) * peak);
    }
}

// ---- a window inside a padded frame (frameio.hip, roiio.hip) -------------------------------------------------------------------------
// One image item of the window of H x W at (top, left) of image b's frame (rows row_pitch floats apart, colour planes plane_pitch)
// -> its samples in the dense integer planes yi [B][H][W], ui and vi [B][H/2][W/2].
template <typename T, bool LVEC, bool SVEC>
__device__ inline void rgb_window_item_to_planes(const float *frame, size_t row_pitch, size_t plane_pitch, int top, int left, int H, int W, size_t b,
                                                 const YuvItem it, double peak, T *__restrict__ yi, T *__restrict__ ui, T *__restrict__ vi)
{
    const int Hc = H >> 1, Wc = W >> 1;
    const size_t plane = (size_t)H * W, cplane = (size_t)Hc * Wc;
    const int nc = it.valid >> 1;                               // chroma samples of this item: 2, or 1
    YuvItemOut<T> o;
    rgb_item_to_yuv420<T, LVEC>(frame + (size_t)(top + 2 * it.cy) * row_pitch + left + it.x0, row_pitch, plane_pitch, it.valid, peak, o);
    const size_t off = b * plane + (size_t)(2 * it.cy) * W + it.x0;
    store_n<SVEC>(yi + off, it.valid, o.yq[0]);
    store_n<SVEC>(yi + off + W, it.valid, o.yq[1]);
    const size_t coff = b * cplane + (size_t)it.cy * Wc + (it.x0 >> 1);
    store_n<SVEC>(ui + coff, nc, o.uq);
    store_n<SVEC>(vi + coff, nc, o.vq);
}

// Pad item p of a frame of Hp x Wp around a window of H x W at (top, left): columns c0 .. c1 (at most four) of row `row`.  The items
// are numbered over the pad alone: first the Hp - H full rows above and below the window in groups of four columns, then, row by row
// of the window, the groups left and right of it (the right ones start at left + W, whatever its alignment).  No element belongs to
// two items and none to no item, so a poisoned pad comes back clean.
struct PadItem {
    int row, c0, c1;
    bool live;
};
__device__ inline PadItem pad_item_at(long long p, int Hp, int Wp, int top, int left, int H, int W)
{
    const int gW = (Wp + 3) >> 2;
    const long long bands = (long long)(Hp - H) * gW;
    PadItem it;
    it.live = true;
    if (p < bands) {                                            // the full rows above and below the window
        const int r = (int)(p / gW);
        it.row = r < top ? r : r + H;
        it.c0 = (int)(p - (long long)r * gW) * 4;
        it.c1 = it.c0 + 4 < Wp ? it.c0 + 4 : Wp;
        return it;
    }
    p -= bands;                                                 // left and right of the window
    const int right0 = left + W, gL = (left + 3) >> 2, gR = (Wp - right0 + 3) >> 2, gs = gL + gR;
    if (gs == 0 || p >= (long long)H * gs) {
        it.live = false, it.row = it.c0 = it.c1 = 0;
        return it;
    }
    const int r = (int)(p / gs), g = (int)(p - (long long)r * gs);
    it.row = top + r;
    if (g < gL) {
        it.c0 = 4 * g;
        it.c1 = it.c0 + 4 < left ? it.c0 + 4 : left;
    } else {
        it.c0 = right0 + 4 * (g - gL);
        it.c1 = it.c0 + 4 < Wp ? it.c0 + 4 : Wp;
    }
    return it;
}

// a pad item's zeros, into each colour plane at o; vec: four aligned columns are one vector per plane
__device__ inline void zero_group(float *o, size_t plane, int n, bool vec)
{
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        store_n<true>(o, 4, z), store_n<true>(o + plane, 4, z), store_n<true>(o + 2 * plane, 4, z);
    } else {
        store_n<false>(o, n, z), store_n<false>(o + plane, n, z), store_n<false>(o + 2 * plane, n, z);
    }
}

// host side: how many pad items `pad_item_at` numbers
inline long long pad_item_count(int Hp, int Wp, int left, int H, int W)
{
    return (long long)(Hp - H) * ((Wp + 3) / 4) + (long long)H * ((left + 3) / 4 + (Wp - left - W + 3) / 4);
}

// host side: the window of H x W at (top, left) lies inside Hp x Wp
inline int window_fits(const char *who, int Hp, int Wp, int top, int left, int H, int W)
{
    STEM_CHECK_ARG(Hp > 0 && Wp > 0 && Hp < (1 << 30) && Wp < (1 << 30), "%s: a frame of %d x %d", who, Hp, Wp);
    STEM_CHECK_ARG(top >= 0 && left >= 0 && top <= Hp - H && left <= Wp - W, "%s: the %d x %d window at (%d, %d) does not fit a frame of %d x %d", who, H,
                   W, top, left, Hp, Wp);
    return 0;
}

// ---- host side: the geometry checks of every entry point; no device needed.  nblk: workgroups per image. ---------------------------
inline int yuv_plan(const char *who, int B, int H, int W, int sample_bytes, int bit_depth, int *nblk)
{
    STEM_CHECK_ARG(B > 0 && B <= 65535, "%s: the batch must be 1 .. 65535 images, got %d", who, B);
    STEM_CHECK_ARG(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "%s: 4:2:0 frames have even sides >= 2, got %d x %d", who, H, W);
    STEM_CHECK_ARG(sample_bytes == 1 || sample_bytes == 2, "%s: samples are 1 or 2 bytes wide, got %d", who, sample_bytes);
    STEM_CHECK_ARG((bit_depth == 8 || bit_depth == 10) && bit_depth <= 8 * sample_bytes, "%s: bit_depth %d in %d-byte samples (8, or 10 in two bytes)", who,
                   bit_depth, sample_bytes);
    const long long items = (long long)(H / 2) * ((W + 3) / 4);
    STEM_CHECK_ARG(items <= (long long)YUV_THREADS * 0x7fffffff, "%s: %d x %d is too large", who, H, W);
    *nblk = (int)((items + YUV_THREADS - 1) / YUV_THREADS);
    return 0;
}

inline bool aligned_to(const void *p, size_t a) { return p == nullptr || (((uintptr_t)p) & (a - 1)) == 0; }

}   // namespace yuv_elem
