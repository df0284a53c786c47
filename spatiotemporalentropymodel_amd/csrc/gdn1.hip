// GDN1 (include/stem_gdn1.h): y = x / (beta' + gamma' |x|), forward and backward, as kernels of their own on the fp32 matrix
// instruction v_mfma_f32_32x32x2_f32 (exact fp32 products, one ascending-k chain per output element).
//
//   walk()            the contraction both pixel-tile kernels share: a workgroup (4 waves) holds a tile of pixels [pixel][channel] in LDS
//                     as the A operand (pixel = MFMA row) and walks all output channels (MFMA column = channel, so one accumulator
//                     register stores as two 128-byte row segments); the B operand is gamma', reparametrised while a 32 x NCH chunk
//                     of the STORED gamma is staged (registers -> LDS, the next chunk's loads in flight under the MFMAs)
//   gdn1_fwd_kernel   64 pixels per workgroup: n = walk(|x|, gamma'^T) + beta', y = x / n | x n
//   gdn1_bwd_kernel   32 pixels per workgroup: n as above, g and u from it (u replaces dy in LDS, g goes to LDS and to the scratch
//                     tensor), then s = walk(g, gamma') and dx = u + sgn(x) s
//   gdn1_wgrad_kernel one partial [C][C] + [C] per STEM_GDN1_PIX_CHUNK pixels: dgamma' = g^T |x| (|x| taken while staged), dbeta' = column
//                     sums of g in pixel order
//   gdn1_tail_kernel  the partials summed in chunk order, then d stored = 2 max(v, bound) d' under the LowerBound rule
#include "stem_common.h"
#include "../../include/stem_gdn1.h"

#include <math.h>

namespace {

constexpr float kPed = 1.4551915228366852e-11f;         // 2^-36
constexpr float kGammaBound = 3.814697265625e-06f;      // 2^-18 = sqrt(0 + 2^-36)
constexpr int NT = 256;                                 // threads per workgroup: 4 waves
constexpr int KC = 32;                                  // k extent of a staged gamma chunk
constexpr int FWD_PG = 2, BWD_PG = 1;                   // 32-pixel groups per workgroup

__device__ __forceinline__ float reparam(float v, float bound)
{
    const float m = fmaxf(v, bound);
    return m * m - kPed;
}
#define GDN1_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0)

__host__ __device__ constexpr int kpad_of(int C) { return (C + KC - 1) / KC * KC; }
__host__ __device__ constexpr int tile_ld(int C) { return kpad_of(C) + 1; }      // odd: the A fragment's 32 rows hit 32 banks
__host__ __device__ constexpr int chunk_ld(int PG) { return 32 * (4 / PG) + 1; }
// floats of LDS: `tiles` pixel tiles of 32 PG rows and the gamma chunk
inline size_t lds_bytes(int C, int PG, int tiles) { return ((size_t)tiles * 32 * PG * tile_ld(C) + (size_t)KC * chunk_ld(PG)) * sizeof(float); }

// rows [p0, p0 + rows) of src (pitch ld) -> dst[rows][LD], columns [0, kpad); pixels past npix and columns past C are zero
template <bool VEC>
__device__ __forceinline__ void stage_tile(float *dst, int LD, int kpad, const float *__restrict__ src, int ld, size_t p0, size_t npix, int rows,
                                           int C)
{
    if (VEC) {
        const int per = kpad >> 2;
        for (int e = threadIdx.x; e < rows * per; e += NT) {
            const int r = e / per, c = (e - r * per) << 2;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (p0 + r < npix && c < C) v = *reinterpret_cast<const f32x4 *>(src + (p0 + r) * (size_t)ld + c);
            float *d = dst + r * LD + c;
            d[0] = v[0], d[1] = v[1], d[2] = v[2], d[3] = v[3];
        }
    } else {
        for (int e = threadIdx.x; e < rows * kpad; e += NT) {
            const int r = e / kpad, c = e - r * kpad;
            dst[r * LD + c] = (p0 + r < npix && c < C) ? src[(p0 + r) * (size_t)ld + c] : 0.f;
        }
    }
}

// acc[pixel][n] = sum_k A[pixel][k] B[k][n] for every block of 32 output channels n, k ascending from an accumulator of zeros.
//   A = atile[pixel][k] (ABS: |.| as the fragment is read);  B[k][n] = gamma'[n][k] (TR false) or gamma'[k][n] (TR true).
// Wave w serves pixel group w % PG and, of every group of NCH = 32 (4 / PG) channels, the block w / PG; epi(first channel of the block,
// acc) runs once per block that holds a channel < C.  Accumulator register v of lane l: pixel (v & 3) + 8 (v >> 2) + 4 (l >> 5) of the
// group, channel l & 31 of the block.  Every thread of the workgroup must call this (barriers inside); atile is read after a barrier.
template <int PG, bool TR, bool ABS, class Epi>
__device__ __forceinline__ void walk(const float *__restrict__ gamma, int C, const float *atile, int LD, float *gs, Epi epi)
{
    constexpr int NG = 4 / PG, NCH = 32 * NG, LDG = NCH + 1, PER = KC * NCH / NT;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, pg = w % PG, nb = w / PG;
    const int nchunks = kpad_of(C) / KC;
    const float *arow = atile + (pg * 32 + (l & 31)) * LD + (l >> 5);
    const float *brow = gs + (l >> 5) * LDG + nb * 32 + (l & 31);
    float pre[PER];
    auto fetch = [&](int n0, int k0) {
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = t + NT * q;
            const int k = TR ? e / NCH : e & (KC - 1), n = TR ? e % NCH : e / KC;      // consecutive threads along gamma's rows
            const int row = TR ? k0 + k : n0 + n, col = TR ? n0 + n : k0 + k;
            pre[q] = (row < C && col < C) ? reparam(gamma[row * C + col], kGammaBound) : 0.f;
        }
    };
    fetch(0, 0);
    for (int n0 = 0; n0 < C; n0 += NCH) {
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
        for (int kc = 0; kc < nchunks; ++kc) {
            __syncthreads();                           // the previous chunk has been read
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int e = t + NT * q;
                const int k = TR ? e / NCH : e & (KC - 1), n = TR ? e % NCH : e / KC;
                gs[k * LDG + n] = pre[q];
            }
            __syncthreads();
            if (kc + 1 < nchunks)
                fetch(n0, (kc + 1) * KC);
            else if (n0 + NCH < C)
                fetch(n0 + NCH, 0);
            const float *a = arow + kc * KC;
#pragma unroll
            for (int kk = 0; kk < KC / 2; ++kk) {
                float av = a[2 * kk];
                if (ABS) av = fabsf(av);
                acc = GDN1_MFMA(av, brow[2 * kk * LDG], acc);
            }
        }
        if (n0 + nb * 32 < C) epi(n0 + nb * 32, acc);
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void gdn1_fwd_kernel(const float *__restrict__ x, int ldx, const float *__restrict__ beta,
                                                      const float *__restrict__ gamma, float *__restrict__ y, int ldy, size_t npix, int C,
                                                      int inverse, float beta_bound)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int LD = tile_ld(C);
    float *xs = smem, *gs = xs + 32 * FWD_PG * LD;
    const size_t p0 = (size_t)blockIdx.x * (32 * FWD_PG);
    stage_tile<VEC>(xs, LD, kpad_of(C), x, ldx, p0, npix, 32 * FWD_PG, C);
    const int l = threadIdx.x & 63, pg = (threadIdx.x >> 6) % FWD_PG;
    walk<FWD_PG, false, true>(gamma, C, xs, LD, gs, [&](int c0, const f32x16 &acc) {
        const int c = c0 + (l & 31);
        if (c >= C) return;
        const float bp = reparam(beta[c], beta_bound);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = pg * 32 + (v & 3) + 8 * (v >> 2) + 4 * (l >> 5);
            if (p0 + r >= npix) continue;
            const float n = acc[v] + bp, xv = xs[r * LD + c];
            y[(p0 + r) * (size_t)ldy + c] = inverse ? xv * n : xv * (1.f / n);
        }
    });
}

// g (scratch, dense [npix][C]) and dx are optional
template <bool VEC>
__global__ __launch_bounds__(NT) void gdn1_bwd_kernel(const float *__restrict__ x, int ldx, const float *__restrict__ dy, int lddy,
                                                      const float *__restrict__ beta, const float *__restrict__ gamma, float *__restrict__ dx,
                                                      int lddx, float *__restrict__ g, size_t npix, int C, int inverse, float beta_bound)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int LD = tile_ld(C), kpad = kpad_of(C);
    float *xs = smem, *ds = xs + 32 * LD, *gt = ds + 32 * LD, *gs = gt + 32 * LD;
    const size_t p0 = (size_t)blockIdx.x * 32;
    stage_tile<VEC>(xs, LD, kpad, x, ldx, p0, npix, 32, C);
    stage_tile<VEC>(ds, LD, kpad, dy, lddy, p0, npix, 32, C);
    for (int e = threadIdx.x; e < 32 * (kpad - C); e += NT) {       // g's columns past C are k steps of the second contraction
        const int r = e / (kpad - C), c = C + e - r * (kpad - C);
        gt[r * LD + c] = 0.f;
    }
    const int l = threadIdx.x & 63;
    walk<BWD_PG, false, true>(gamma, C, xs, LD, gs, [&](int c0, const f32x16 &acc) {
        const int c = c0 + (l & 31);
        if (c >= C) return;
        const float bp = reparam(beta[c], beta_bound);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = (v & 3) + 8 * (v >> 2) + 4 * (l >> 5);
            const float n = acc[v] + bp, xv = xs[r * LD + c], dv = ds[r * LD + c];
            float u, gv;
            if (inverse) {
                u = dv * n;
                gv = dv * xv;
            } else {
                const float rn = 1.f / n;
                u = dv * rn;
                gv = -(dv * xv) * (rn * rn);
            }
            ds[r * LD + c] = u;                        // read back by this thread only
            gt[r * LD + c] = gv;
            if (g && p0 + r < npix) g[(p0 + r) * (size_t)C + c] = gv;
        }
    });
    if (!dx) return;
    walk<BWD_PG, true, false>(gamma, C, gt, LD, gs, [&](int c0, const f32x16 &acc) {
        const int c = c0 + (l & 31);
        if (c >= C) return;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = (v & 3) + 8 * (v >> 2) + 4 * (l >> 5);
            if (p0 + r >= npix) continue;
            const float xv = xs[r * LD + c];
            const float sg = xv > 0.f ? 1.f : (xv < 0.f ? -1.f : 0.f);
            dx[(p0 + r) * (size_t)lddx + c] = fmaf(sg, acc[v], ds[r * LD + c]);
        }
    });
}

// partial[chunk][i][j] = sum over the chunk's pixels, ascending, of g[p][i] |x[p][j]|; partial[chunk][C * C + i] = sum of g[p][i].
// grid (chunks, tiles): a workgroup owns a T x T tile of [i][j], T = 64 WB; wave w the WB x WB blocks of 32 x 32 at (w & 1, w >> 1).
template <int WB, bool VEC>
__global__ __launch_bounds__(NT) void gdn1_wgrad_kernel(const float *__restrict__ g, const float *__restrict__ x, int ldx, float *__restrict__ part,
                                                        size_t npix, int C)
{
    constexpr int T = 64 * WB;
    __shared__ __attribute__((aligned(16))) float ga[32 * T], xb[32 * T];
    const int tiles = (C + T - 1) / T, ti = blockIdx.y / tiles, tj = blockIdx.y - ti * tiles, i0 = ti * T, j0 = tj * T;
    const size_t pbeg = (size_t)blockIdx.x * STEM_GDN1_PIX_CHUNK;
    const size_t pend = pbeg + STEM_GDN1_PIX_CHUNK < npix ? pbeg + STEM_GDN1_PIX_CHUNK : npix;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, wi = (w & 1) * WB, wj = (w >> 1) * WB;
    f32x16 acc[WB][WB];
#pragma unroll
    for (int a = 0; a < WB; ++a)
#pragma unroll
        for (int b = 0; b < WB; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.f;
    float bsum = 0.f;
    for (size_t p = pbeg; p < pend; p += 32) {
        __syncthreads();
        if (VEC) {
            for (int e = t; e < 32 * (T / 4); e += NT) {
                const int r = e / (T / 4), c = (e - r * (T / 4)) << 2;
                f32x4 gv = {0.f, 0.f, 0.f, 0.f}, xv = gv;
                if (p + r < pend && i0 + c < C) gv = *reinterpret_cast<const f32x4 *>(g + (p + r) * (size_t)C + i0 + c);
                if (p + r < pend && j0 + c < C) xv = *reinterpret_cast<const f32x4 *>(x + (p + r) * (size_t)ldx + j0 + c);
#pragma unroll
                for (int q = 0; q < 4; ++q) xv[q] = fabsf(xv[q]);
                *reinterpret_cast<f32x4 *>(ga + r * T + c) = gv;
                *reinterpret_cast<f32x4 *>(xb + r * T + c) = xv;
            }
        } else {
            for (int e = t; e < 32 * T; e += NT) {
                const int r = e / T, c = e - r * T;
                ga[e] = (p + r < pend && i0 + c < C) ? g[(p + r) * (size_t)C + i0 + c] : 0.f;
                xb[e] = (p + r < pend && j0 + c < C) ? fabsf(x[(p + r) * (size_t)ldx + j0 + c]) : 0.f;
            }
        }
        __syncthreads();
        if (tj == 0 && t < T) {
#pragma unroll 8
            for (int r = 0; r < 32; ++r) bsum += ga[r * T + t];
        }
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            const int k = 2 * kk + (l >> 5);
            float av[WB], bv[WB];
#pragma unroll
            for (int a = 0; a < WB; ++a) av[a] = ga[k * T + (wi + a) * 32 + (l & 31)];
#pragma unroll
            for (int b = 0; b < WB; ++b) bv[b] = xb[k * T + (wj + b) * 32 + (l & 31)];
#pragma unroll
            for (int a = 0; a < WB; ++a)
#pragma unroll
                for (int b = 0; b < WB; ++b) acc[a][b] = GDN1_MFMA(av[a], bv[b], acc[a][b]);
        }
    }
    float *out = part + (size_t)blockIdx.x * ((size_t)C * C + C);
    if (tj == 0 && t < T && i0 + t < C) out[(size_t)C * C + i0 + t] = bsum;
#pragma unroll
    for (int a = 0; a < WB; ++a)
#pragma unroll
        for (int b = 0; b < WB; ++b) {
            const int j = j0 + (wj + b) * 32 + (l & 31);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = i0 + (wi + a) * 32 + (v & 3) + 8 * (v >> 2) + 4 * (l >> 5);
                if (i < C && j < C) out[(size_t)i * C + j] = acc[a][b][v];
            }
        }
}

// element e of [C][C] (gamma) then [C] (beta): d' = the partials summed in chunk order; d stored under the LowerBound rule
__global__ __launch_bounds__(NT) void gdn1_tail_kernel(const float *__restrict__ part, size_t nchunks, const float *__restrict__ beta,
                                                       const float *__restrict__ gamma, float *__restrict__ dbeta, float *__restrict__ dgamma,
                                                       int C, float beta_bound)
{
    const int n = C * C + C, e = blockIdx.x * NT + threadIdx.x;
    if (e >= n) return;
    float d = 0.f;
    for (size_t c = 0; c < nchunks; ++c) d += part[c * (size_t)n + e];
    const bool isg = e < C * C;
    const float raw = isg ? gamma[e] : beta[e - C * C], bound = isg ? kGammaBound : beta_bound;
    const float gr = 2.f * fmaxf(raw, bound) * d;
    const float o = (raw >= bound || gr < 0.f) ? gr : 0.f;
    if (isg)
        dgamma[e] = o;
    else
        dbeta[e - C * C] = o;
}

inline bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }
inline bool vec_ok(const void *ptr, int ld) { return !ptr || (ld % 4 == 0 && aligned16(ptr)); }
inline float beta_bound_of(float beta_min) { return (float)sqrt((double)beta_min + 1.4551915228366852e-11); }
inline size_t g_elems(size_t npix, int C) { return (npix * (size_t)C + 3) / 4 * 4; }
inline size_t n_chunks(size_t npix) { return cdivz(npix, STEM_GDN1_PIX_CHUNK); }

}   // namespace

STEM_EXPORT int stem_gdn1_fwd(const float *x, int ldx, const float *beta, const float *gamma, float *y, int ldy, size_t npix, int C, int inverse,
                              float beta_min, void *stream)
{
    if (npix == 0) return 0;
    STEM_CHECK_ARG(C > 0 && C <= STEM_GDN1_MAX_C, "stem_gdn1_fwd: C = %d is outside 1 .. %d", C, STEM_GDN1_MAX_C);
    STEM_CHECK_ARG(x && beta && gamma && y, "stem_gdn1_fwd: null pointer");
    STEM_CHECK_ARG(ldx >= C && ldy >= C, "stem_gdn1_fwd: a pixel pitch (%d %d) is smaller than C = %d", ldx, ldy, C);
    const size_t nblk = cdivz(npix, 32 * FWD_PG);
    STEM_CHECK_ARG(nblk <= 0x7FFFFFFFu, "stem_gdn1_fwd: %zu pixels exceed one grid", npix);
    const bool vec = C % 4 == 0 && vec_ok(x, ldx);
    const size_t lds = lds_bytes(C, FWD_PG, 1);
    static const hipError_t attr[2] = {
        hipFuncSetAttribute((const void *)gdn1_fwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(STEM_GDN1_MAX_C, FWD_PG, 1)),
        hipFuncSetAttribute((const void *)gdn1_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(STEM_GDN1_MAX_C, FWD_PG, 1))};
    (void)attr;
    hipLaunchKernelGGL(vec ? gdn1_fwd_kernel<true> : gdn1_fwd_kernel<false>, dim3((unsigned)nblk), dim3(NT), lds, (hipStream_t)stream, x, ldx, beta,
                       gamma, y, ldy, npix, C, inverse ? 1 : 0, beta_bound_of(beta_min));
    STEM_LAUNCH_CHECK("gdn1_fwd");
    return 0;
}

STEM_EXPORT size_t stem_gdn1_bwd_workspace_bytes(size_t npix, int C)
{
    if (npix == 0 || C <= 0 || C > STEM_GDN1_MAX_C) return 0;
    return (g_elems(npix, C) + n_chunks(npix) * ((size_t)C * C + C)) * sizeof(float);
}

STEM_EXPORT int stem_gdn1_bwd(const float *x, int ldx, const float *dy, int lddy, const float *beta, const float *gamma, float *dx, int lddx,
                              float *dbeta, float *dgamma, size_t npix, int C, int inverse, float beta_min, void *ws, size_t ws_bytes,
                              void *stream)
{
    if (npix == 0) return 0;
    STEM_CHECK_ARG(C > 0 && C <= STEM_GDN1_MAX_C, "stem_gdn1_bwd: C = %d is outside 1 .. %d", C, STEM_GDN1_MAX_C);
    STEM_CHECK_ARG(x && dy && beta && gamma, "stem_gdn1_bwd: null pointer");
    STEM_CHECK_ARG(dx || dbeta || dgamma, "stem_gdn1_bwd: no output: dx, dbeta and dgamma are all NULL");
    STEM_CHECK_ARG(!dbeta == !dgamma, "stem_gdn1_bwd: dbeta and dgamma go together");
    STEM_CHECK_ARG(ldx >= C && lddy >= C && (!dx || lddx >= C), "stem_gdn1_bwd: a pixel pitch (%d %d %d) is smaller than C = %d", ldx, lddy, lddx,
                   C);
    const bool params = dgamma != nullptr;
    const size_t need = stem_gdn1_bwd_workspace_bytes(npix, C);
    STEM_CHECK_ARG(!params || (ws && ws_bytes >= need), "stem_gdn1_bwd: workspace too small (%zu < %zu)", ws ? ws_bytes : (size_t)0, need);
    STEM_CHECK_ARG(!params || aligned16(ws), "stem_gdn1_bwd: the workspace is not 16-byte aligned");
    const size_t nblk = cdivz(npix, 32 * BWD_PG);
    STEM_CHECK_ARG(nblk <= 0x7FFFFFFFu, "stem_gdn1_bwd: %zu pixels exceed one grid", npix);
    hipStream_t st = (hipStream_t)stream;
    float *g = params ? (float *)ws : nullptr, *part = params ? g + g_elems(npix, C) : nullptr;
    const float bb = beta_bound_of(beta_min);
    const bool vec = C % 4 == 0 && vec_ok(x, ldx) && vec_ok(dy, lddy);
    const size_t lds = lds_bytes(C, BWD_PG, 3);
    static const hipError_t attr[2] = {
        hipFuncSetAttribute((const void *)gdn1_bwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(STEM_GDN1_MAX_C, BWD_PG, 3)),
        hipFuncSetAttribute((const void *)gdn1_bwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(STEM_GDN1_MAX_C, BWD_PG, 3))};
    (void)attr;
    hipLaunchKernelGGL(vec ? gdn1_bwd_kernel<true> : gdn1_bwd_kernel<false>, dim3((unsigned)nblk), dim3(NT), lds, st, x, ldx, dy, lddy, beta, gamma,
                       dx, lddx, g, npix, C, inverse ? 1 : 0, bb);
    STEM_LAUNCH_CHECK("gdn1_bwd");
    if (!params) return 0;
    const int WB = C > 64 ? 2 : 1, T = 64 * WB, tiles = cdiv(C, T);
    const bool vecw = C % 4 == 0 && vec_ok(x, ldx);         // g is dense at the workspace's aligned base
    const dim3 grid((unsigned)n_chunks(npix), (unsigned)(tiles * tiles));
    auto wgrad = WB == 2 ? (vecw ? gdn1_wgrad_kernel<2, true> : gdn1_wgrad_kernel<2, false>)
                         : (vecw ? gdn1_wgrad_kernel<1, true> : gdn1_wgrad_kernel<1, false>);
    hipLaunchKernelGGL(wgrad, grid, dim3(NT), 0, st, g, x, ldx, part, npix, C);
    STEM_LAUNCH_CHECK("gdn1_wgrad");
    hipLaunchKernelGGL(gdn1_tail_kernel, dim3((unsigned)cdiv(C * C + C, NT)), dim3(NT), 0, st, part, n_chunks(npix), beta, gamma, dbeta, dgamma, C, bb);
    STEM_LAUNCH_CHECK("gdn1_tail");
    return 0;
}
