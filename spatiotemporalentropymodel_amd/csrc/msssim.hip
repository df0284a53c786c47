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

// ---- backward: d ms_ssim[b] / d x ------------------------------------------------------------------------------------------------
// The function differentiated is exactly the one above.  With m_{s,c} the clamped mean of scale s and channel c and
// P_c = prod_s m_{s,c}^{w_s}, d ms / d m_{s,c} = w_s P_c / (C m_{s,c}); a channel with any clamped term has P_c = 0 and a gradient
// of exactly 0.  Per scale, with f the per-pixel cs (ssim on scale 5) as a function of the window means mu1 = G[x], e11 = G[x*x],
// e12 = G[x*y], the gradient at that scale's resolution is  G^T[k f_mu1] + 2x G^T[k f_e11] + y G^T[k f_e12]  (k = grad_ms[b] *
// d ms / d m / number of filtered pixels; G^T the "full" correlation with the same window) plus the pooling adjoint of the coarser
// scale's gradient: pixel (r, c) takes a quarter of coarse pixel ((r + H % 2) / 2, (c + W % 2) / 2).
//
// One launch per scale, coarse to fine; a 512-thread workgroup owns one 32 x 32 tile of one plane of that scale's gradient:
//   1. the 52 x 52 halo of x and y (origin 10 above / left of the tile) goes to LDS, zero beyond the plane;
//   2. horizontal pass of the five quantities, 52 rows x 42 columns, fp64 -> LDS;
//   3. vertical pass on the 42 x 42 ring of filtered pixels the tile's adjoint reaches, the three coefficient maps in fp64 -> LDS
//      (zero where the ring leaves the filtered map);
//   4. adjoint vertical pass (42 -> 32 rows, over the memory of step 2), adjoint horizontal pass in registers;
//   5. + a quarter of the coarser scale's gradient; one plain store per pixel (fp64 planes of scales 2-5 in the workspace, fp32 dx).
// Every LDS index is linear in the work-item number: fp64 rows are read 32 consecutive doubles per half-wave, one bank row.
// No atomics; nothing depends on the batch around an image.
namespace {

constexpr int MB_THREADS = 512;
constexpr int MB_RING = MS_T + MS_TAPS - 1;        // 42: filtered pixels per side that reach the tile
constexpr int MB_HALO = MB_RING + MS_TAPS - 1;     // 52: input pixels per side under that ring
constexpr int MB_PITCH = MB_HALO + 1;              // 53 floats

struct MsBwdScale {
    int H, W;                                      // plane size at this scale
    int nty, ntx;                                  // tiles of the H x W gradient plane
    int scale;                                     // 0 .. 4
};

// per plane and scale: grad_ms[b] * w_s * P_c / (C * m_{s,c} * count_s); 0 for every scale of a channel with a clamped term
struct MsInvCount {
    double v[MS_SCALES];
};
__global__ __launch_bounds__(256) void msssim_bwd_coef_kernel(const double *__restrict__ mean, const float *__restrict__ grad_ms, int planes,
                                                              int C, MsInvCount inv, double *__restrict__ coef)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= planes) return;
    double m[MS_SCALES], prod = 1.0;
    bool alive = true;
#pragma unroll
    for (int s = 0; s < MS_SCALES; ++s) {
        m[s] = mean[(size_t)p * MS_SCALES + s];
        alive = alive && m[s] > 0.0;
        prod *= pow(m[s], kExponent[s]);
    }
    const double g = (double)grad_ms[p / C];
    double k[MS_SCALES];
#pragma unroll
    for (int s = 0; s < MS_SCALES; ++s) {
        k[s] = alive ? g * kExponent[s] * prod * inv.v[s] / ((double)C * m[s]) : 0.0;
        alive = alive && isfinite(k[s]);
    }
#pragma unroll
    for (int s = 0; s < MS_SCALES; ++s) coef[(size_t)p * MS_SCALES + s] = alive ? k[s] : 0.0;
}

// derivatives of cs (scales 1-4) or ssim (scale 5) of one pixel with respect to mu1, e11, e12.  Contraction off, as in ssim_pixel.
template <bool FULL>
__device__ inline void ssim_pixel_grad(double mu1, double mu2, double e11, double e22, double e12, double C1, double C2, double &d_mu1,
                                       double &d_e11, double &d_e12)
{
#pragma clang fp contract(off)
    const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
    const double s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
    const double den = (s11 + s22) + C2, cs = (2.0 * s12 + C2) / den;
    const double c_mu1 = 2.0 * (cs * mu1 - mu2) / den, c_e11 = -cs / den, c_e12 = 2.0 / den;
    if (!FULL) {
        d_mu1 = c_mu1;
        d_e11 = c_e11;
        d_e12 = c_e12;
        return;
    }
    const double lden = (m11 + m22) + C1, l = (2.0 * m12 + C1) / lden;
    const double l_mu1 = 2.0 * (mu2 - l * mu1) / lden;
    d_mu1 = l_mu1 * cs + l * c_mu1;
    d_e11 = l * c_e11;
    d_e12 = l * c_e12;
}

// x, y: [planes][H][W] of this scale; coef: [planes][5]; gc: [planes][(H+1)/2][(W+1)/2] fp64 gradient of the next scale (COARSE);
// out: [planes][H][W], fp64 (workspace) or fp32 (dx)
template <bool FULL, bool COARSE, typename OutT>
__global__ __launch_bounds__(MB_THREADS) void msssim_bwd_scale_kernel(const float *__restrict__ x, const float *__restrict__ y, MsBwdScale sc,
                                                                      MsWindow win, double C1, double C2, const double *__restrict__ coef,
                                                                      const double *__restrict__ gc, OutT *__restrict__ out)
{
    __shared__ float xs[MB_HALO][MB_PITCH], ys[MB_HALO][MB_PITCH];
    __shared__ double hb[5 * MB_HALO * MB_RING];                       // [5][52][42]; later the adjoint's [3][32][42]
    __shared__ double qm[3][MB_RING][MB_RING];

    const int ntiles = sc.nty * sc.ntx;
    const int plane = blockIdx.x / ntiles, tile = blockIdx.x - plane * ntiles;
    const int ty = tile / sc.ntx, tx = tile - ty * sc.ntx;
    const int H = sc.H, W = sc.W, Ho = H - (MS_TAPS - 1), Wo = W - (MS_TAPS - 1);
    const int oy0 = ty * MS_T, ox0 = tx * MS_T;
    const int hy0 = oy0 - (MS_TAPS - 1), hx0 = ox0 - (MS_TAPS - 1);   // origin of the halo and of the ring
    const float *xp = x + (size_t)plane * H * W, *yp = y + (size_t)plane * H * W;
    const double k = coef[(size_t)plane * MS_SCALES + sc.scale];      // the same for the whole workgroup

    double acc[2][3];                                                  // the three adjoints of this thread's two pixels
#pragma unroll
    for (int o = 0; o < 2; ++o) acc[o][0] = acc[o][1] = acc[o][2] = 0.0;

    if (k != 0.0) {
        // 1. halo -> LDS, zero beyond the plane (those pixels only feed ring positions that are masked out in step 3)
        for (int i = threadIdx.x; i < MB_HALO * MB_HALO; i += MB_THREADS) {
            const int r = i / MB_HALO, c = i - r * MB_HALO;
            const int gy = hy0 + r, gx = hx0 + c;
            const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const size_t g = ok ? (size_t)gy * W + gx : 0;
            xs[r][c] = ok ? xp[g] : 0.f;
            ys[r][c] = ok ? yp[g] : 0.f;
        }
        __syncthreads();

        double w[MS_TAPS];
#pragma unroll
        for (int t = 0; t < MS_TAPS; ++t) w[t] = (double)win.w[t];

        // 2. horizontal pass, as the forward's: 52 rows x 42 columns of the five quantities
        for (int i = threadIdx.x; i < MB_HALO * MB_RING; i += MB_THREADS) {
            const int r = i / MB_RING, c = i - r * MB_RING;
            double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
            for (int t = 0; t < MS_TAPS; ++t) {
                const double xv = (double)xs[r][c + t], yv = (double)ys[r][c + t];
                a += w[t] * xv;
                b += w[t] * yv;
                aa += w[t] * (xv * xv);
                bb += w[t] * (yv * yv);
                ab += w[t] * (xv * yv);
            }
            hb[0 * MB_HALO * MB_RING + i] = a;
            hb[1 * MB_HALO * MB_RING + i] = b;
            hb[2 * MB_HALO * MB_RING + i] = aa;
            hb[3 * MB_HALO * MB_RING + i] = bb;
            hb[4 * MB_HALO * MB_RING + i] = ab;
        }
        __syncthreads();

        // 3. vertical pass on the ring; k * (f_mu1, f_e11, f_e12), zero outside the filtered map
        for (int i = threadIdx.x; i < MB_RING * MB_RING; i += MB_THREADS) {
            const int r = i / MB_RING, c = i - r * MB_RING;
            double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < MS_TAPS; ++t)
#pragma unroll
                for (int q = 0; q < 5; ++q) v[q] += w[t] * hb[q * MB_HALO * MB_RING + i + t * MB_RING];
            const int my = hy0 + r, mx = hx0 + c;
            const bool ok = my >= 0 && my < Ho && mx >= 0 && mx < Wo;
            double d0, d1, d2;
            ssim_pixel_grad<FULL>(v[0], v[1], v[2], v[3], v[4], C1, C2, d0, d1, d2);
            qm[0][r][c] = ok ? k * d0 : 0.0;
            qm[1][r][c] = ok ? k * d1 : 0.0;
            qm[2][r][c] = ok ? k * d2 : 0.0;
        }
        __syncthreads();

        // 4a. adjoint, vertical: output row ro takes ring rows ro .. ro + 10 with the window reversed -> [3][32][42] over hb
        for (int i = threadIdx.x; i < MS_T * MB_RING; i += MB_THREADS) {
            double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < MS_TAPS; ++t)
#pragma unroll
                for (int q = 0; q < 3; ++q) v[q] += w[MS_TAPS - 1 - t] * (&qm[q][0][0])[i + t * MB_RING];
#pragma unroll
            for (int q = 0; q < 3; ++q) hb[q * MS_T * MB_RING + i] = v[q];
        }
        __syncthreads();

        // 4b. adjoint, horizontal: two pixels per thread, 16 rows apart
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const int i = threadIdx.x + o * MB_THREADS, r = i >> 5, c = i & 31;
#pragma unroll
            for (int t = 0; t < MS_TAPS; ++t)
#pragma unroll
                for (int q = 0; q < 3; ++q) acc[o][q] += w[MS_TAPS - 1 - t] * hb[q * MS_T * MB_RING + r * MB_RING + c + t];
        }
    }

    // 5. the pixel's own factors, the pooled adjoint, one store
    const int padh = H & 1, padw = W & 1, Wp = (W + 1) >> 1;
    const size_t cplane = (size_t)plane * ((H + 1) >> 1) * Wp;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const int i = threadIdx.x + o * MB_THREADS, r = i >> 5, c = i & 31;
        const int gy = oy0 + r, gx = ox0 + c;
        if (gy >= H || gx >= W) continue;
        double g = 0.0;
        if (k != 0.0) {
#pragma clang fp contract(off)
            const double xv = (double)xs[r + MS_TAPS - 1][c + MS_TAPS - 1], yv = (double)ys[r + MS_TAPS - 1][c + MS_TAPS - 1];
            g = (acc[o][0] + (2.0 * xv) * acc[o][1]) + yv * acc[o][2];
        }
        if (COARSE) g += 0.25 * gc[cplane + (size_t)((gy + padh) >> 1) * Wp + ((gx + padw) >> 1)];
        out[(size_t)plane * H * W + (size_t)gy * W + gx] = (OutT)g;
    }
}

// the backward's workspace: the coefficients, then the fp64 gradient planes of scales 2-5
struct MsBwdPlan {
    MsBwdScale sc[MS_SCALES];
    size_t coef, grad[MS_SCALES], bytes;
};

int ms_bwd_plan(const char *who, int B, int C, const MsPlan &f, MsBwdPlan *p)
{
    const size_t planes = (size_t)B * C;
    size_t off = 0;
    p->coef = off;
    off += align256(planes * MS_SCALES * sizeof(double));
    for (int s = 0; s < MS_SCALES; ++s) {
        const int h = f.sc[s].H, w = f.sc[s].W;
        p->sc[s] = {h, w, cdiv(h, MS_T), cdiv(w, MS_T), s};
        STEM_CHECK_ARG(planes * p->sc[s].nty * p->sc[s].ntx < (size_t)1 << 31, "%s: [%d,%d,%d,%d] is too large", who, B, C, f.sc[0].H, f.sc[0].W);
        p->grad[s] = off;
        if (s) off += align256(planes * h * w * sizeof(double));
    }
    p->bytes = off;
    return 0;
}

}   // namespace

STEM_EXPORT int stem_ms_ssim_bwd_workspace(int B, int C, int H, int W, size_t *bytes)
{
    STEM_CHECK_ARG(bytes, "stem_ms_ssim_bwd_workspace: null pointer");
    MsPlan f;
    if (int rc = ms_plan("stem_ms_ssim_bwd_workspace", B, C, H, W, &f)) return rc;
    MsBwdPlan p;
    if (int rc = ms_bwd_plan("stem_ms_ssim_bwd_workspace", B, C, f, &p)) return rc;
    *bytes = p.bytes;
    return 0;
}

STEM_EXPORT int stem_ms_ssim_bwd(const float *x, const float *y, int B, int C, int H, int W, float data_range, const void *fwd_workspace,
                                 size_t fwd_workspace_bytes, const float *grad_ms, void *workspace, size_t workspace_bytes, float *dx,
                                 void *stream)
{
    STEM_CHECK_ARG(x && y && fwd_workspace && grad_ms && workspace && dx, "stem_ms_ssim_bwd: null pointer");
    STEM_CHECK_ARG(data_range > 0.f, "stem_ms_ssim_bwd: data_range must be positive, got %g", (double)data_range);
    MsPlan f;
    if (int rc = ms_plan("stem_ms_ssim_bwd", B, C, H, W, &f)) return rc;
    MsBwdPlan p;
    if (int rc = ms_bwd_plan("stem_ms_ssim_bwd", B, C, f, &p)) return rc;
    STEM_CHECK_ARG(fwd_workspace_bytes >= f.bytes, "stem_ms_ssim_bwd: forward workspace of %zu bytes, %zu needed (stem_ms_ssim_workspace)",
                   fwd_workspace_bytes, f.bytes);
    STEM_CHECK_ARG(workspace_bytes >= p.bytes, "stem_ms_ssim_bwd: workspace of %zu bytes, %zu needed (stem_ms_ssim_bwd_workspace)", workspace_bytes,
                   p.bytes);
    STEM_CHECK_ARG(((((uintptr_t)workspace) | ((uintptr_t)fwd_workspace)) & 7) == 0, "stem_ms_ssim_bwd: workspaces must be 8-byte aligned");

    const char *fws = static_cast<const char *>(fwd_workspace);
    char *ws = static_cast<char *>(workspace);
    const int planes = B * C;
    const double C1 = (0.01 * (double)data_range) * (0.01 * (double)data_range), C2 = (0.03 * (double)data_range) * (0.03 * (double)data_range);
    hipStream_t st = (hipStream_t)stream;
    double *coef = reinterpret_cast<double *>(ws + p.coef);
    MsInvCount inv;
    for (int s = 0; s < MS_SCALES; ++s) inv.v[s] = 1.0 / ((double)(f.sc[s].H - (MS_TAPS - 1)) * (double)(f.sc[s].W - (MS_TAPS - 1)));
    hipLaunchKernelGGL(msssim_bwd_coef_kernel, dim3(cdiv(planes, 256)), dim3(256), 0, st, reinterpret_cast<const double *>(fws + f.mean), grad_ms,
                       planes, C, inv, coef);
    STEM_LAUNCH_CHECK("stem_ms_ssim_bwd");
    for (int s = MS_SCALES - 1; s >= 0; --s) {
        const MsBwdScale &sc = p.sc[s];
        const size_t plane_bytes = align256((size_t)planes * sc.H * sc.W * sizeof(float));
        const float *xs = s ? reinterpret_cast<const float *>(fws + f.pyr[s]) : x;
        const float *ys = s ? reinterpret_cast<const float *>(fws + f.pyr[s] + plane_bytes) : y;
        const double *gc = s + 1 < MS_SCALES ? reinterpret_cast<const double *>(ws + p.grad[s + 1]) : nullptr;
        const dim3 grid((unsigned)(planes * sc.nty * sc.ntx)), block(MB_THREADS);
        if (s == MS_SCALES - 1)
            hipLaunchKernelGGL((msssim_bwd_scale_kernel<true, false, double>), grid, block, 0, st, xs, ys, sc, kWindow, C1, C2, coef, gc,
                               reinterpret_cast<double *>(ws + p.grad[s]));
        else if (s)
            hipLaunchKernelGGL((msssim_bwd_scale_kernel<false, true, double>), grid, block, 0, st, xs, ys, sc, kWindow, C1, C2, coef, gc,
                               reinterpret_cast<double *>(ws + p.grad[s]));
        else
            hipLaunchKernelGGL((msssim_bwd_scale_kernel<false, true, float>), grid, block, 0, st, xs, ys, sc, kWindow, C1, C2, coef, gc, dx);
        STEM_LAUNCH_CHECK("stem_ms_ssim_bwd");
    }
    return 0;
}
