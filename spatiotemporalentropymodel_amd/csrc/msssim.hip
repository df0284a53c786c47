// MS-SSIM and mean squared error of two fp32 NCHW image batches (stem/evalSTEM.py:81,147 and :29-31): the arithmetic of
// evaluation.ms_ssim -- five scales, separable 11-tap Gaussian window (sigma 1.5, normalised in float64, rounded to fp32),
// "valid" filtering of x, y, x*x, y*y, x*y, K = (0.01, 0.03), 2x2 average pooling with padding s % 2 between scales.
//
// One launch per scale.  A 256-thread workgroup owns one 32 x 32 tile of the filtered map of one (image, channel) plane:
//   1. the 42 x 42 halo of x and y goes to LDS (zero beyond the plane);
//   2. the tile's share of the 2x2-pooled planes of the next scale is written from that image (fp32, summed in torch's order);
//      on scale 1 the tile's share of sum (x - y)^2 is taken from it as well;
//   3. horizontal pass: the five quantities, 42 rows x 32 columns, accumulated in fp64 (x*x, x*y are exact there) -> LDS;
//   4. vertical pass in fp64, four consecutive rows per thread from a sliding 14-row window; cs / ssim per pixel in fp64;
//   5. the tile's sum, reduced in a fixed order, goes to the workgroup's own fp64 slot with a plain store.
// A finaliser (one workgroup per image) sums the slots in a fixed order, clamps, raises to the exponents and averages the
// channels.  No atomics anywhere: the result is bit-identical from run to run and does not depend on the batch around an image.
// Every expression that mixes x and y is evaluated without fused contraction, so ms_ssim(x, y) == ms_ssim(y, x) bit for bit.
#include "stem_common.h"

#include <math.h>

namespace {

constexpr int MS_T = 32;                          // tile side (filtered pixels)
constexpr int MS_TAPS = 11;
constexpr int MS_HALO = MS_T + MS_TAPS - 1;       // 42 input rows / columns per tile
constexpr int MS_PITCH = MS_HALO + 1;             // 43 floats: odd, rows of one wave fall on different banks
constexpr int MS_SCALES = 5;
constexpr int MS_THREADS = 256;
constexpr int MS_MIN_SIDE = (MS_TAPS - 1) << (MS_SCALES - 1);      // 160: a side must be LARGER than this

// evaluation._gauss_window(): exp(-c^2 / (2 * 1.5^2)), c = -5 .. 5, normalised in float64, rounded to fp32 (taps 0 .. 5; symmetric)
struct MsWindow {
    float w[MS_TAPS];
};
const MsWindow kWindow = {{0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f, 0x1.b43c4p-3f,
                           0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}};
// exponents of the five scales (Wang, Simoncelli, Bovik 2003)
__constant__ double kExponent[MS_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};

struct MsScale {                                   // one scale of one call
    int H, W;                                      // plane size at this scale
    int nty, ntx;                                  // tiles of the (H - 10) x (W - 10) filtered map
};

// sum over the workgroup in a fixed order (256 threads); every thread gets it
__device__ inline double block_sum(double v, double *red)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// cs (scales 1-4) or ssim (scale 5) of one pixel from the five window means.  Contraction off: a fused multiply-add would round
// mu1*mu1 + mu2*mu2 differently from mu2*mu2 + mu1*mu1.
template <bool FULL>
__device__ inline double ssim_pixel(double mu1, double mu2, double e11, double e22, double e12, double C1, double C2)
{
#pragma clang fp contract(off)
    const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
    const double s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
    const double cs = (2.0 * s12 + C2) / ((s11 + s22) + C2);
    if (!FULL) return cs;
    return (2.0 * m12 + C1) / ((m11 + m22) + C1) * cs;
}

// x, y: [planes][H][W] of this scale.  xn, yn: [planes][(H+1)/2][(W+1)/2] of the next one (POOL).  part: [planes][nty*ntx] sums of
// the map; sq: the same shape, sums of (x - y)^2 over the input pixels a tile owns (MSE: scale 1 only).
template <bool POOL, bool MSE, bool FULL>
__global__ __launch_bounds__(MS_THREADS) void msssim_scale_kernel(const float *__restrict__ x, const float *__restrict__ y, MsScale sc,
                                                                  MsWindow win, double C1, double C2, float *__restrict__ xn,
                                                                  float *__restrict__ yn, double *__restrict__ part, double *__restrict__ sq)
{
    __shared__ float xs[MS_HALO][MS_PITCH], ys[MS_HALO][MS_PITCH];
    __shared__ double hb[5][MS_HALO][MS_T];
    __shared__ double red[4];

    const int ntiles = sc.nty * sc.ntx;
    const int plane = blockIdx.x / ntiles, tile = blockIdx.x - plane * ntiles;
    const int ty = tile / sc.ntx, tx = tile - ty * sc.ntx;
    const int H = sc.H, W = sc.W, Ho = H - (MS_TAPS - 1), Wo = W - (MS_TAPS - 1);
    const int oy0 = ty * MS_T, ox0 = tx * MS_T;
    const bool lasty = ty == sc.nty - 1, lastx = tx == sc.ntx - 1;
    const float *xp = x + (size_t)plane * H * W, *yp = y + (size_t)plane * H * W;

    // 1. halo -> LDS, zero beyond the plane (those rows / columns only feed filtered pixels that are masked out below)
    for (int i = threadIdx.x; i < MS_HALO * MS_HALO; i += MS_THREADS) {
        const int r = i / MS_HALO, c = i - r * MS_HALO;
        const int gy = oy0 + r, gx = ox0 + c;
        const bool ok = gy < H && gx < W;
        const size_t g = ok ? (size_t)gy * W + gx : 0;
        xs[r][c] = ok ? xp[g] : 0.f;
        ys[r][c] = ok ? yp[g] : 0.f;
    }
    __syncthreads();

    // the input rows / columns this tile owns: its 32, and everything up to the edge for the last tile of a row / column
    const int ownh = lasty ? H - oy0 : MS_T, ownw = lastx ? W - ox0 : MS_T;      // <= MS_HALO

    // 2a. sum (x - y)^2 over the owned input pixels (differences and squares of fp32 values are exact in fp64)
    if (MSE) {
        double s = 0.0;
        for (int i = threadIdx.x; i < ownh * ownw; i += MS_THREADS) {
            const int r = i / ownw, c = i - r * ownw;
            const double d = (double)xs[r][c] - (double)ys[r][c];
            s += d * d;
        }
        s = block_sum(s, red);
        if (threadIdx.x == 0) sq[blockIdx.x] = s;
    }

    // 2b. avg_pool2d(kernel_size=2, padding=s % 2): pooled pixel (py, px) covers input rows 2*py - padh, 2*py - padh + 1 (row -1 is the
    // zero padding, the divisor stays 4).  A tile owns the pooled pixels whose FIRST row and column it owns; the second ones
    // are in its halo.  Summed as torch does: row by row, left to right.
    if (POOL) {
        const int padh = H & 1, padw = W & 1, Hp = (H + 1) >> 1, Wp = (W + 1) >> 1;
        const int py0 = ty == 0 ? 0 : (oy0 + padh + 1) >> 1, py1 = lasty ? Hp : (oy0 + MS_T + padh + 1) >> 1;
        const int px0 = tx == 0 ? 0 : (ox0 + padw + 1) >> 1, px1 = lastx ? Wp : (ox0 + MS_T + padw + 1) >> 1;
        const int nph = py1 - py0, npw = px1 - px0;
        float *xo = xn + (size_t)plane * Hp * Wp, *yo = yn + (size_t)plane * Hp * Wp;
        for (int i = threadIdx.x; i < nph * npw; i += MS_THREADS) {
            const int pr = i / npw, pc = i - pr * npw;
            const int py = py0 + pr, px = px0 + pc;
            const int r0 = 2 * py - padh - oy0, c0 = 2 * px - padw - ox0;       // -1 only for the padding row / column of the plane
            const bool rv = r0 >= 0, cv = c0 >= 0;
            const int r0c = rv ? r0 : 0, c0c = cv ? c0 : 0;
            const float x00 = rv && cv ? xs[r0c][c0c] : 0.f, x01 = rv ? xs[r0c][c0 + 1] : 0.f, x10 = cv ? xs[r0 + 1][c0c] : 0.f;
            const float y00 = rv && cv ? ys[r0c][c0c] : 0.f, y01 = rv ? ys[r0c][c0 + 1] : 0.f, y10 = cv ? ys[r0 + 1][c0c] : 0.f;
            xo[(size_t)py * Wp + px] = (((x00 + x01) + x10) + xs[r0 + 1][c0 + 1]) * 0.25f;
            yo[(size_t)py * Wp + px] = (((y00 + y01) + y10) + ys[r0 + 1][c0 + 1]) * 0.25f;
        }
    }

    double w[MS_TAPS];
#pragma unroll
    for (int k = 0; k < MS_TAPS; ++k) w[k] = (double)win.w[k];

    // 3. horizontal pass: 42 rows x 32 columns; one wave reads two rows of 32 + 10 consecutive floats (conflict-free)
    for (int i = threadIdx.x; i < MS_HALO * MS_T; i += MS_THREADS) {
        const int r = i >> 5, c = i & 31;
        double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
        for (int k = 0; k < MS_TAPS; ++k) {
            const double xv = (double)xs[r][c + k], yv = (double)ys[r][c + k];
            a += w[k] * xv;
            b += w[k] * yv;
            aa += w[k] * (xv * xv);
            bb += w[k] * (yv * yv);
            ab += w[k] * (xv * yv);
        }
        hb[0][r][c] = a;
        hb[1][r][c] = b;
        hb[2][r][c] = aa;
        hb[3][r][c] = bb;
        hb[4][r][c] = ab;
    }
    __syncthreads();

    // 4. vertical pass: thread = one column, four consecutive rows, 14 window rows read once each
    const int c = threadIdx.x & 31, rb = (threadIdx.x >> 5) * 4;
    double acc[4][5];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[o][q] = 0.0;
#pragma unroll
    for (int r = 0; r < MS_TAPS + 3; ++r) {
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = hb[q][rb + r][c];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = r - o;
            if (k >= 0 && k < MS_TAPS) {
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[o][q] += w[k] * v[q];
            }
        }
    }
    double s = 0.0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const bool ok = oy0 + rb + o < Ho && ox0 + c < Wo;
        const double m = ssim_pixel<FULL>(acc[o][0], acc[o][1], acc[o][2], acc[o][3], acc[o][4], C1, C2);
        s += ok ? m : 0.0;
    }
    // 5. the tile's sum -> its own slot
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

struct MsFinal {
    const double *part[MS_SCALES];                 // [planes][ntiles[s]]
    int ntiles[MS_SCALES];
    double inv_count[MS_SCALES];                   // 1 / ((H_s - 10) * (W_s - 10))
    const double *sq;                              // [planes][ntiles[0]]
    double inv_pixels;                             // 1 / (C * H * W)
};

// One workgroup per image.  Wave w sums the slots of (channel, scale) pairs w, w + 4, ... lane-strided, then across lanes: a
// fixed order.  `mean`: [B][C][5] doubles of workspace (clamped means); thread 0 forms the product and the channel mean.
__global__ __launch_bounds__(MS_THREADS) void msssim_final_kernel(MsFinal f, int C, double *__restrict__ mean, float *__restrict__ out,
                                                                  float *__restrict__ mse, float *__restrict__ terms)
{
    __shared__ double red[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = wave; p < C * MS_SCALES; p += MS_THREADS / 64) {
        const int ch = p / MS_SCALES, s = p - ch * MS_SCALES;
        const double *src = f.part[s] + (size_t)(b * C + ch) * f.ntiles[s];
        double v = 0.0;
        for (int i = lane; i < f.ntiles[s]; i += 64) v += src[i];
#pragma unroll
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) {
            const double m = fmax(v * f.inv_count[s], 0.0);
            mean[(size_t)(b * C + ch) * MS_SCALES + s] = m;
            if (terms) terms[(size_t)(b * C + ch) * MS_SCALES + s] = (float)m;
        }
    }
    double q = 0.0;
    if (mse) {
        const double *src = f.sq + (size_t)b * C * f.ntiles[0];
        for (int i = threadIdx.x; i < C * f.ntiles[0]; i += MS_THREADS) q += src[i];
    }
    __threadfence_block();
    q = block_sum(q, red);                         // its barriers also order the `mean` stores before thread 0's loads
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int ch = 0; ch < C; ++ch) {
            double prod = 1.0;
            for (int s = 0; s < MS_SCALES; ++s) prod *= pow(mean[(size_t)(b * C + ch) * MS_SCALES + s], kExponent[s]);
            sum += prod;
        }
        out[b] = (float)(sum / C);
        if (mse) mse[b] = (float)(q * f.inv_pixels);
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the workspace of one call: pooled x / y planes of scales 2-5, the slots of the five scales and of the MSE, the clamped means
struct MsPlan {
    MsScale sc[MS_SCALES];
    size_t pyr[MS_SCALES];                         // byte offset of the x planes of scale s (s >= 1); the y planes follow them
    size_t part[MS_SCALES], sq, mean, bytes;
};

// argument checks shared by the two entry points; no device needed
int ms_plan(const char *who, int B, int C, int H, int W, MsPlan *p)
{
    STEM_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "%s: non-positive shape [%d,%d,%d,%d]", who, B, C, H, W);
    STEM_CHECK_ARG((H < W ? H : W) > MS_MIN_SIDE, "%s: %d x %d frames have no fifth scale (the smaller side must exceed %d)", who, H, W, MS_MIN_SIDE);
    const size_t planes = (size_t)B * C;
    size_t off = 0;
    int h = H, w = W;
    for (int s = 0; s < MS_SCALES; ++s) {
        p->sc[s] = {h, w, cdiv(h - (MS_TAPS - 1), MS_T), cdiv(w - (MS_TAPS - 1), MS_T)};
        STEM_CHECK_ARG(planes * p->sc[s].nty * p->sc[s].ntx < (size_t)1 << 31 && planes * h * w < (size_t)1 << 40, "%s: [%d,%d,%d,%d] is too large", who, B, C, H, W);
        p->pyr[s] = off;
        if (s) off += 2 * align256(planes * h * w * sizeof(float));
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    for (int s = 0; s < MS_SCALES; ++s) {
        p->part[s] = off;
        off += align256(planes * p->sc[s].nty * p->sc[s].ntx * sizeof(double));
    }
    p->sq = off;
    off += align256(planes * p->sc[0].nty * p->sc[0].ntx * sizeof(double));
    p->mean = off;
    off += align256(planes * MS_SCALES * sizeof(double));
    p->bytes = off;
    return 0;
}

}   // namespace

STEM_EXPORT int stem_ms_ssim_workspace(int B, int C, int H, int W, size_t *bytes)
{
    STEM_CHECK_ARG(bytes, "stem_ms_ssim_workspace: null pointer");
    MsPlan p;
    if (int rc = ms_plan("stem_ms_ssim_workspace", B, C, H, W, &p)) return rc;
    *bytes = p.bytes;
    return 0;
}

STEM_EXPORT int stem_ms_ssim(const float *x, const float *y, int B, int C, int H, int W, float data_range, void *workspace,
                             size_t workspace_bytes, float *ms_ssim, float *mse, float *terms, void *stream)
{
    STEM_CHECK_ARG(x && y && workspace && ms_ssim, "stem_ms_ssim: null pointer");
    STEM_CHECK_ARG(data_range > 0.f, "stem_ms_ssim: data_range must be positive, got %g", (double)data_range);
    MsPlan p;
    if (int rc = ms_plan("stem_ms_ssim", B, C, H, W, &p)) return rc;
    STEM_CHECK_ARG(workspace_bytes >= p.bytes, "stem_ms_ssim: workspace of %zu bytes, %zu needed (stem_ms_ssim_workspace)", workspace_bytes, p.bytes);
    STEM_CHECK_ARG((((uintptr_t)workspace) & 7) == 0, "stem_ms_ssim: workspace must be 8-byte aligned");

    char *ws = static_cast<char *>(workspace);
    const int planes = B * C;
    const double C1 = (0.01 * (double)data_range) * (0.01 * (double)data_range), C2 = (0.03 * (double)data_range) * (0.03 * (double)data_range);
    hipStream_t st = (hipStream_t)stream;
    MsFinal f;
    for (int s = 0; s < MS_SCALES; ++s) {
        const MsScale &sc = p.sc[s];
        const size_t plane_bytes = align256((size_t)planes * sc.H * sc.W * sizeof(float));
        const float *xs = s ? reinterpret_cast<const float *>(ws + p.pyr[s]) : x;
        const float *ys = s ? reinterpret_cast<const float *>(ws + p.pyr[s] + plane_bytes) : y;
        float *xn = nullptr, *yn = nullptr;
        if (s + 1 < MS_SCALES) {
            const MsScale &nx = p.sc[s + 1];
            xn = reinterpret_cast<float *>(ws + p.pyr[s + 1]);
            yn = reinterpret_cast<float *>(ws + p.pyr[s + 1] + align256((size_t)planes * nx.H * nx.W * sizeof(float)));
        }
        double *part = reinterpret_cast<double *>(ws + p.part[s]), *sq = reinterpret_cast<double *>(ws + p.sq);
        const int ntiles = sc.nty * sc.ntx;
        const dim3 grid((unsigned)(planes * ntiles)), block(MS_THREADS);
        if (s == 0)
            hipLaunchKernelGGL((msssim_scale_kernel<true, true, false>), grid, block, 0, st, xs, ys, sc, kWindow, C1, C2, xn, yn, part, sq);
        else if (s + 1 < MS_SCALES)
            hipLaunchKernelGGL((msssim_scale_kernel<true, false, false>), grid, block, 0, st, xs, ys, sc, kWindow, C1, C2, xn, yn, part, sq);
        else
            hipLaunchKernelGGL((msssim_scale_kernel<false, false, true>), grid, block, 0, st, xs, ys, sc, kWindow, C1, C2, xn, yn, part, sq);
        STEM_LAUNCH_CHECK("stem_ms_ssim");
        f.part[s] = part;
        f.ntiles[s] = ntiles;
        f.inv_count[s] = 1.0 / ((double)(sc.H - (MS_TAPS - 1)) * (double)(sc.W - (MS_TAPS - 1)));
    }
    f.sq = reinterpret_cast<const double *>(ws + p.sq);
    f.inv_pixels = 1.0 / ((double)C * H * W);
    hipLaunchKernelGGL(msssim_final_kernel, dim3(B), dim3(MS_THREADS), 0, st, f, C, reinterpret_cast<double *>(ws + p.mean), ms_ssim, mse, terms);
    STEM_LAUNCH_CHECK("stem_ms_ssim");
    return 0;
}
