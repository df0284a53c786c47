// Producers of the split-operand fp16 family's operands (f16x3_layout.h) that are not convolutions: the maximum passes that feed
// the scale records, fp32 NHWC <-> planes (split, split with the leaky-ReLU derivative, merge) and the weight packs -- one tensor
// (wide or gen image), every layer's image with one launch, both images of every layer from one read of its weights.
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "f16x3_layout.h"

namespace {

// max |x| of an NHWC tensor (rows of C floats at pitch ldx) -> one slot per workgroup of the record q: the pass in front of a
// split whose input no kernel of this library has measured
__global__ __launch_bounds__(256) void amax_nhwc_kernel(const float *x, int ldx, long npix, int c4n, float *q)
{
    __shared__ float qred[16];
    float m = 0.f;
    const long n4 = npix * c4n;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long)gridDim.x * 256) {
        const long pix = e / c4n;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(x + pix * ldx + (e - pix * c4n) * 4);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    m = block_max(m, qred);
    if (threadIdx.x == 0) {
        q[QREC_HDR + blockIdx.x] = m;
        if (blockIdx.x == 0) q_header(q, gridDim.x);
    }
}

// the same for flat fp32 arrays (weights), blockIdx.y = tensor
struct AmaxTable {
    float *w[24];
    float *q[24];
    long n[24];
    short rs[24], taps[24];        // taps > 0: a masked convolution -- taps >= taps[i] of every filter are ZEROED IN PLACE (what the
                                   // reference does at every forward: layers.py:44 `self.weight.data *= self.mask`) and not counted
};
__global__ __launch_bounds__(256) void amax_multi_kernel(const AmaxTable tab)
{
    __shared__ float qred[16];
    float *w = tab.w[blockIdx.y];
    const long n = tab.n[blockIdx.y];
    float m = 0.f;
    const long stride = (long)gridDim.x * 256;
    long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (tab.taps[blockIdx.y] > 0) {
        const int rs = tab.rs[blockIdx.y], live = tab.taps[blockIdx.y];
        for (; e < n; e += stride) {
            if ((int)(e % rs) >= live)
                w[e] = 0.f;
            else
                m = fmaxf(m, fabsf(w[e]));
        }
    }
    // eight independent loads in flight per thread (a flat parameter buffer guarantees 4-byte alignment only: scalar loads)
    for (; e + 7 * stride < n; e += 8 * stride) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = w[e + u * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) m = fmaxf(m, fabsf(v[u]));
    }
    for (; e < n; e += stride) m = fmaxf(m, fabsf(w[e]));
    m = block_max(m, qred);
    if (threadIdx.x == 0) {
        float *q = tab.q[blockIdx.y];
        q[QREC_HDR + blockIdx.x] = m;
        if (blockIdx.x == 0) q_header(q, gridDim.x);
    }
}

// fp32 NHWC -> planes: one thread per (pixel, slab, 8-channel piece)
// DACT: x * (z > 0 ? 1 : slope) -> planes: the gradient that reaches a convolution whose output was activated (z = that output),
// split for the fp16 input-gradient / weight-gradient kernels in the pass that applies the leaky-ReLU derivative
template <bool DACT>
__global__ __launch_bounds__(256) void split_nhwc_kernel(const float *x, int ldx, const float *z, int ldz, float slope, unsigned char *xp,
                                                         long npieces, int nslab, float *q, const float *qsrc)
{
    // qsrc: the record whose slots hold max |x| -- q itself (amax_nhwc_kernel ran on it) or the record of the kernel that produced x
    __shared__ float qred[16];
    float xmax = q_amax(qsrc, qred);
    if constexpr (DACT) xmax *= fmaxf(1.f, fabsf(slope));
    const int xe = q_exp(xmax);
    const float xscale = q_pow2(xe);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        q[1] = q_pow2(-xe);
        if (qsrc != q) {
            q_header(q, 1);
            q[QREC_HDR] = xmax;
        }
    }
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= npieces) return;
    const long pix = e / (nslab * 4);
    const int rem = (int)(e - pix * (nslab * 4)), sl = rem >> 2, p = rem & 3;
    const float *src = x + pix * ldx + sl * 32 + p * 8;
    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(src), v1 = *reinterpret_cast<const f32x4 *>(src + 4);
    f32x4 z0 = v0, z1 = v1;
    if constexpr (DACT) {
        const float *zs = z + pix * ldz + sl * 32 + p * 8;
        z0 = *reinterpret_cast<const f32x4 *>(zs), z1 = *reinterpret_cast<const f32x4 *>(zs + 4);
    }
    h16x8 h0, h1;
    q_split8([&](int c) {
        const float v = c < 4 ? v0[c] : v1[c - 4];
        return !DACT || (c < 4 ? z0[c] : z1[c - 4]) > 0.f ? v : v * slope;
    }, xscale, h0, h1);
    unsigned char *dst = planes_piece(xp, pix, nslab, sl, p);
    *reinterpret_cast<h16x8 *>(dst) = h0;
    *reinterpret_cast<h16x8 *>(dst + PLANE1) = h1;
}

// planes -> fp32 NHWC (tests / debugging): the two planes add up to the fp32 value exactly
__global__ __launch_bounds__(256) void merge_planes_kernel(const unsigned char *xp, float *x, int ldx, long nelem, int C, const float *q)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nelem) return;
    const long pix = e / C;
    const int c = (int)(e - pix * C), sl = c >> 5, k = c & 31;
    const hp_t *src = reinterpret_cast<const hp_t *>(planes_piece(xp, pix, C / 32, sl, 0));
    x[pix * ldx + c] = ((float)src[k] + (float)src[PLANE1 / 2 + k]) * q_inv(q);
}

// torch Conv2d weight [N][C][R][S] fp32 -> one weight image of ROWS rows per N tile: GBN (gen image) or BN (wide image: one tile).
// flip: the input-gradient of a stride-1 convolution is a convolution of dy with w'[c][k][r][s] = w[k][c][R-1-r][S-1-s]: `w` is
// still the torch weight [K][C][R][S], the packed rows are its input channels c (N = C outputs) and the packed channels its
// output channels k.
// T <= RS: only the first T taps (row-major) are packed -- the live taps of a type-A / type-B masked convolution (layers.py:21-47)
template <int ROWS>
__global__ __launch_bounds__(256) void pack_weight_kernel(const float *w, unsigned char *wp, int N, int C, int RS, int T, int flip, long npieces,
                                                          float *wq)
{
    __shared__ float qred[16];
    const int we = q_exp(q_amax(wq, qred));
    const float wscale = q_pow2(we);
    if (blockIdx.x == 0 && threadIdx.x == 0) wq[1] = q_pow2(-we);
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= npieces) return;
    const int nchunks = (C / 32) * T;
    const int p = (int)(e & 3), nl = (int)((e >> 2) % ROWS);
    const long qq = e / (4 * ROWS);                      // ntile * nchunks + q
    const int ntile = ROWS == BN ? 0 : (int)(qq / nchunks), q = (int)(qq - (long)ntile * nchunks);      // the wide image is one tile
    const int slab = q / T, tap = q - slab * T, n = ntile * ROWS + nl;
    h16x8 h[NPL];
    q_split8([&](int c) {
        const int ch = slab * 32 + p * 8 + c;
        float v = 0.f;
        if (n < N) v = flip ? w[((size_t)ch * N + n) * RS + (RS - 1 - tap)] : w[((size_t)n * C + ch) * RS + tap];
        return v;
    }, wscale, h[0], h[1]);
    unsigned char *dst = wimg_piece(wp + qq * (NPL * ROWS * 64), nl, p);
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) *reinterpret_cast<h16x8 *>(dst + pl * (ROWS * 64)) = h[pl];
}

// every layer's weight image with one launch: blockIdx.y = descriptor (the weights of a training model change every step).  The
// table travels by value in the kernel arguments: no staging buffer whose lifetime would have to outlast the queued launch.
constexpr int MAXPACK = 24;
struct PackTable {
    stem_f16x2_pack_desc d[MAXPACK];
};
constexpr int PKR = 8;                                  // output rows per unit
__global__ __launch_bounds__(256) void pack_weight_gen_multi_kernel(const PackTable tab)
{
    // One workgroup per unit = (8 consecutive output rows n, one 32-channel slab), grid-strided.  The 8 x 32 x RS source values
    // of a unit are read in long contiguous runs of the torch weight -- forward role: per row n the slab's 32 x RS values are
    // one run; flip role (rows = input channels of the forward layer): per contraction channel the 8 rows' RS values are one
    // run -- into LDS, then every thread emits whole 16-byte pieces (8 channels of one tap and row, both planes).  (The first
    // version handled one row per unit: 100-byte runs in flip mode and two barriers per 800 values.)
    __shared__ float tile[PKR * 32 * MAXTAP];         // [row][channel in slab][tap]
    const stem_f16x2_pack_desc &d = tab.d[blockIdx.y];
    const int nslab = d.C / 32, ntile = cdiv_dev(d.N, GBN);
    const float *w = static_cast<const float *>(d.w);
    unsigned char *wp = static_cast<unsigned char *>(d.wp);
    float *wq = reinterpret_cast<float *>(wp + (size_t)ntile * nslab * d.R * d.S * GB_BUF);    // the scale record sits behind the FULL image's size
    __shared__ float qred[16];
    float wmax;
    if (d.bmax) {       // maxima of the optimiser pass's chunks that cover this tensor (an upper bound: neighbours may share a chunk)
        float mm = 0.f;
        for (int i = threadIdx.x; i < 4 * d.nb; i += 256) mm = fmaxf(mm, d.bmax[4 * d.b0 + i]);      // four wavefront maxima per chunk
        wmax = block_max(mm, qred);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            q_header(wq, 1);
            wq[QREC_HDR] = wmax;
        }
    } else {
        wmax = q_amax(wq, qred);                                                       // amax_multi_kernel ran
    }
    const int we = q_exp(wmax);
    const float wscale = q_pow2(we);
    if (blockIdx.x == 0 && threadIdx.x == 0) wq[1] = q_pow2(-we);
    float *wz = (d.bmax && d.taps > 0 && d.taps < d.R * d.S) ? static_cast<float *>(const_cast<void *>(d.w)) : nullptr;      // masked taps zeroed here (no maximum pass did it)
    // flip == 2: the four phase images of a transposed face (tconv_slot): transposed indexing like the flip role, taps permuted into
    // phase order, one image per phase behind the other (sum of the phases' taps = RS: the record sits where it always does)
    __shared__ int pslot[MAXTAP], pT[4], pbase[4];
    if (d.flip == 2) {
        if (threadIdx.x < d.R * d.S) pslot[threadIdx.x] = tconv_slot(d.R, d.S, d.R / 2, threadIdx.x / d.S, threadIdx.x % d.S);
        if (threadIdx.x < 4) {
            int b = 0;
            for (int p = 0; p < (int)threadIdx.x; ++p) b += tconv_axis(d.R, d.R / 2, p >> 1).cnt * tconv_axis(d.S, d.S / 2, p & 1).cnt;
            pbase[threadIdx.x] = b;
            pT[threadIdx.x] = tconv_axis(d.R, d.R / 2, threadIdx.x >> 1).cnt * tconv_axis(d.S, d.S / 2, threadIdx.x & 1).cnt;
        }
        __syncthreads();
    }
    const int units = ntile * (GBN / PKR) * nslab;
    // the element loops divide by RS and 32 RS / PKR RS per element: with the window size a compile-time constant (1, 9, 25: every
    // layer of the model) those are multiplications -- the pass is bound by its index arithmetic, not by HBM, otherwise
    auto run = [&](auto rs_const) {
        constexpr int CRS = decltype(rs_const)::value;
        const int RS = CRS > 0 ? CRS : d.R * d.S;
        const int T = d.taps > 0 ? d.taps : RS, nchunks = nslab * T;
        for (int u = blockIdx.x; u < units; u += gridDim.x) {
            const int slab = u % nslab, n0 = (u / nslab) * PKR;   // n runs over the padded rows of all N tiles
            __syncthreads();
            if (d.flip) {
                // element (row r, channel c, tap): w[((slab * 32 + c) * N + n0 + r) * RS + (RS - 1 - tap)]: for fixed c, PKR * RS contiguous floats
                for (int e = threadIdx.x; e < 32 * PKR * RS; e += 256) {
                    const int c = e / (PKR * RS), rem = e - c * (PKR * RS), r = rem / RS, tp = rem - r * RS;
                    const int n = n0 + r;
                    tile[(r * 32 + c) * MAXTAP + (d.flip == 2 ? pslot[tp] : RS - 1 - tp)] = n < d.N ? w[((size_t)(slab * 32 + c) * d.N + n) * RS + tp] : 0.f;
                }
            } else {
                // element (row r, channel c, tap): w[((n0 + r) * C + slab * 32 + c) * RS + tap]: for fixed r, 32 * RS contiguous floats
                for (int e = threadIdx.x; e < PKR * 32 * RS; e += 256) {
                    const int r = e / (32 * RS), rem = e - r * (32 * RS), c = rem / RS, tp = rem - c * RS;
                    const int n = n0 + r;
                    const size_t wi = ((size_t)n * d.C + slab * 32 + c) * RS + tp;
                    float wv = n < d.N ? w[wi] : 0.f;
                    if (wz && tp >= T && n < d.N) {
                        wz[wi] = 0.f;
                        wv = 0.f;
                    }
                    tile[(r * 32 + c) * MAXTAP + tp] = wv;
                }
            }
            __syncthreads();
            for (int e = threadIdx.x; e < PKR * T * 4; e += 256) {
                const int p = e & 3, r = (e >> 2) % PKR, tap = (e >> 2) / PKR;
                const int n = n0 + r, nt = n / GBN, nl = n - nt * GBN;
                h16x8 h[NPL];
                q_split8([&](int c) { return tile[(r * 32 + p * 8 + c) * MAXTAP + tap]; }, wscale, h[0], h[1]);
                long qq = (long)nt * nchunks + slab * T + tap;
                if (d.flip == 2) {            // image of phase ph: [N tile][slab * T_ph + local tap], behind the earlier phases' images
                    const int ph = tap >= pbase[3] ? 3 : (tap >= pbase[2] ? 2 : (tap >= pbase[1] ? 1 : 0));
                    qq = (long)ntile * nslab * pbase[ph] + (long)nt * (nslab * pT[ph]) + slab * pT[ph] + (tap - pbase[ph]);
                }
                unsigned char *dst = wimg_piece(wp + qq * GB_BUF, nl, p);
    #pragma unroll
                for (int pl = 0; pl < NPL; ++pl) *reinterpret_cast<h16x8 *>(dst + pl * GB_PLANE) = h[pl];
            }
        }
    };
    const int rs_rt = d.R * d.S;
    if (rs_rt == 25)
        run(std::integral_constant<int, 25>{});
    else if (rs_rt == 9)
        run(std::integral_constant<int, 9>{});
    else if (rs_rt == 1)
        run(std::integral_constant<int, 1>{});
    else
        run(std::integral_constant<int, 0>{});
}

// ---- both weight images of a layer from ONE read of its weights (round 5) ---------------------------------------------------------
// The training step re-packs every weight after every optimiser step (stem/trainSTEM.py:213: the weights changed), once per ROLE:
// the forward image and the input-gradient image of a layer are two transposes of the same numbers.  pack_weight_gen_multi_kernel
// makes one image per descriptor: 72 MB read + 72 MB written per role, 82 + 108 us per P-frame step, the second on the
// weight-gradient stream where it competes with the forward's kernels for HBM.  Here a workgroup takes a 32 x 32 x RS tile
// [a][b][tap] of the torch tensor [A][B][R][S] into LDS once and emits the pieces of BOTH images from it: rows = the tile's a
// index with 8 consecutive b per 16-byte piece (a Conv2d's forward image, a ConvTranspose2d's input-gradient image), or rows = b
// with 8 consecutive a (transposed indexing: flip / phases), taps in identity, mirrored or phase order.
constexpr int PAIR_T = 32;                              // tile edge (channels)
constexpr int PAIR_NT = 512;
constexpr int PAIR_PAD = 4;                             // floats added to the LDS pitch of a tile row (bank spread, see pair_pack_tile)
struct PairRole {
    void *wp;                 // null: the layer has no image of this role
    int rows_b;               // 0: image rows = the tensor's leading index a (contraction over b); 1: rows = b (contraction over a)
    int tapmode;              // 0 identity, 1 mirrored (input gradient of a stride-1 convolution), 2 sub-pixel phase order (tconv_slot)
    int taps;                 // identity only: > 0 = the image holds the first `taps` taps, the others are ZEROED in w (masked convolution)
};
struct PairDesc {
    float *w;
    int A, B, R, S;
    PairRole role[2];
    const float *bmax;        // per-chunk maxima of the optimiser pass (stem_adam_step_bmax) covering the tensor: chunks b0 .. b0 + nb - 1
    int b0, nb;
    int tile0;                // first workgroup of this tensor in the launch
};
constexpr int MAXPAIR = 20;
struct PairTable {
    PairDesc d[MAXPAIR];
    int n;
};

// TA = rows a of the tile: 32, or 16 for 5 x 5 windows (51 KB of LDS instead of 102: three workgroups per CU instead of one --
// the pass is HBM-bound and a lone workgroup per CU alternates between loading and storing)
__host__ __device__ inline int pair_ta(int RS) { return RS > 16 ? 16 : PAIR_T; }      // (8 for 5x5 and 16 for 3x3 measured 66.0 against 64.6 us)
template <int CRS, int TA>
__device__ inline void pair_pack_tile(const PairDesc &d, int tile, float *lds, int *ptap, float wscale)
{
    const int RS = CRS > 0 ? CRS : d.R * d.S;
    const int tb = cdiv_dev(d.B, PAIR_T);
    const int a0 = (tile / tb) * TA, b0 = (tile % tb) * PAIR_T;
    const int na = d.A - a0 < TA ? d.A - a0 : TA, nb = d.B - b0 < PAIR_T ? d.B - b0 : PAIR_T;
    const int row = PAIR_T * RS;                       // floats of one a-row of the tile (b-major, taps innermost): the tensor's own order
    // LDS pitch of an a-row: 32 * RS floats are a multiple of 32 banks for every window (25, 9, 1), so the emission's readers --
    // lanes = (piece p, row rr) -- all hit the banks of ONE row: 16-way conflicts.  Four more floats per row keep the float4
    // stores aligned and spread the 16 rows of a wavefront over eight bank groups
    const int lrow = row + PAIR_PAD;
    // masked convolution: the taps beyond the live prefix are zeroed IN PLACE (layers.py:44 `weight.data *= mask` at every forward)
    const int live = (d.role[0].wp && d.role[0].tapmode == 0 && d.role[0].taps > 0 && d.role[0].taps < RS) ? d.role[0].taps : RS;
    if (na == TA && nb == PAIR_T && live == RS && (reinterpret_cast<uintptr_t>(d.w) & 15) == 0 && ((size_t)d.B * RS) % 4 == 0) {
        // full tile: every a-row of the tile is 32 * RS consecutive floats starting on a 16-byte boundary -- float4 loads, four
        // independent ones in flight per thread
        constexpr int U = 4;
        const int row4 = row / 4, n4 = TA * row4;                      // 32 * RS is a multiple of 4
        for (int base = threadIdx.x; base < n4; base += U * PAIR_NT) {
            f32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i4 = base + u * PAIR_NT;
                const int a = i4 / row4, r4 = i4 - a * row4;
                v[u] = i4 < n4 ? *reinterpret_cast<const f32x4 *>(d.w + ((size_t)(a0 + a) * d.B + b0) * RS + 4 * r4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i4 = base + u * PAIR_NT;
                if (i4 < n4) {
                    const int a = i4 / row4, r4 = i4 - a * row4;
                    *reinterpret_cast<f32x4 *>(lds + a * lrow + 4 * r4) = v[u];
                }
            }
        }
    } else {
        for (int idx = threadIdx.x; idx < TA * row; idx += PAIR_NT) {
            const int a = idx / row, rem = idx - a * row;
            float v = 0.f;
            if (a < na && rem < nb * RS) {
                float *src = d.w + ((size_t)(a0 + a) * d.B + b0) * RS + rem;
                v = *src;
                if (live < RS && rem % RS >= live) {
                    *src = 0.f;
                    v = 0.f;
                }
            }
            lds[a * lrow + rem] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int ri = 0; ri < 2; ++ri) {
        const PairRole &r = d.role[ri];
        if (!r.wp) continue;
        unsigned char *wp = static_cast<unsigned char *>(r.wp);
        const int N = r.rows_b ? d.B : d.A, C = r.rows_b ? d.A : d.B;           // image rows / contraction channels
        const int n0 = r.rows_b ? b0 : a0, nrows = r.rows_b ? nb : na, slab = (r.rows_b ? a0 : b0) / 32;
        const int nslab = C / 32, ntile = cdiv_dev(N, GBN);
        const int T = (r.tapmode == 0 && r.taps > 0) ? r.taps : RS;
        const int nchunks = nslab * T;
        int pT[4] = {0, 0, 0, 0}, pbase[4] = {0, 0, 0, 0};
        if (r.tapmode == 2) {
            int acc = 0;
            for (int p = 0; p < 4; ++p) {
                pbase[p] = acc;
                pT[p] = tconv_axis(d.R, d.R / 2, p >> 1).cnt * tconv_axis(d.S, d.S / 2, p & 1).cnt;
                acc += pT[p];
            }
        }
        // pieces of this tile in the image: rows = a: TA rows x 4 pieces (the tile's 32 b are one contraction slab); rows = b: 32 rows x
        // TA / 8 pieces (the tile's TA a are pieces pofs .. of their slab)
        const int ppr = r.rows_b ? TA / 8 : 4, prow = r.rows_b ? PAIR_T : TA;
        const int pofs = r.rows_b ? (a0 & 31) >> 3 : 0;
        for (int e = threadIdx.x; e < prow * ppr * T; e += PAIR_NT) {
            const int pp = e % ppr, rr = (e / ppr) % prow, tap = e / (ppr * prow);      // piece, row of the tile, image tap
            if (rr >= nrows) continue;
            const int p = pofs + pp;
            // source tap of image tap `tap`: identity, mirrored, or the tap that sits at phase-ordered position `tap`
            const int st = r.tapmode == 0 ? tap : (r.tapmode == 1 ? RS - 1 - tap : ptap[tap]);
            h16x8 h[NPL];
#pragma unroll
            for (int c = 0; c < 8; ++c) {      // (written out: through q_split8 the two tile orientations compile to 6 % more instructions)
                const int ch = pp * 8 + c;                                     // contraction channel inside the tile
                const float v = r.rows_b ? lds[ch * lrow + rr * RS + st] : lds[rr * lrow + ch * RS + st];
                hp_t x0, x1;
                q_split(v, wscale, x0, x1);
                h[0][c] = x0; h[1][c] = x1;
            }
            const int n = n0 + rr, nt = n / GBN, nl = n - nt * GBN;
            long qq = (long)nt * nchunks + slab * T + tap;
            if (r.tapmode == 2) {
                const int ph = tap >= pbase[3] ? 3 : (tap >= pbase[2] ? 2 : (tap >= pbase[1] ? 1 : 0));
                qq = (long)ntile * nslab * pbase[ph] + (long)nt * (nslab * pT[ph]) + slab * pT[ph] + (tap - pbase[ph]);
            }
            unsigned char *dst = wimg_piece(wp + qq * GB_BUF, nl, p);
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) *reinterpret_cast<h16x8 *>(dst + pl * GB_PLANE) = h[pl];
        }
    }
}

__global__ __launch_bounds__(PAIR_NT) void pack_weight_pair_multi_kernel(const PairTable tab)
{
    extern __shared__ __attribute__((aligned(16))) float pair_lds[];            // [32][32][RS] floats, then the phase tap table
    __shared__ float qred[16];
    int i = 0;
    while (i + 1 < tab.n && (int)blockIdx.x >= tab.d[i + 1].tile0) ++i;
    const PairDesc &d = tab.d[i];
    const int tile = blockIdx.x - d.tile0, RS = d.R * d.S;
    int *ptap = reinterpret_cast<int *>(pair_lds + pair_ta(RS) * (PAIR_T * RS + PAIR_PAD));
    if ((int)threadIdx.x < RS) ptap[tconv_slot(d.R, d.S, d.R / 2, threadIdx.x / d.S, threadIdx.x % d.S)] = threadIdx.x;
    // one scale for both images: the maximum of the optimiser pass's chunks that cover the tensor (an upper bound: neighbours may
    // share a chunk), as in pack_weight_gen_multi_kernel
    float mm = 0.f;
    for (int k = threadIdx.x; k < 4 * d.nb; k += PAIR_NT) mm = fmaxf(mm, d.bmax[4 * d.b0 + k]);
    const float wmax = block_max(mm, qred);
    const int we = q_exp(wmax);
    if (tile == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int ri = 0; ri < 2; ++ri) {
            const PairRole &r = d.role[ri];
            if (!r.wp) continue;
            const int N = r.rows_b ? d.B : d.A, C = r.rows_b ? d.A : d.B;
            float *wq = reinterpret_cast<float *>(static_cast<unsigned char *>(r.wp) + (size_t)cdiv_dev(N, GBN) * (C / 32) * RS * GB_BUF);
            q_header(wq, 1);
            wq[1] = q_pow2(-we);
            wq[QREC_HDR] = wmax;
        }
    }
    __syncthreads();
    const float wscale = q_pow2(we);
    if (RS == 25)
        pair_pack_tile<25, 16>(d, tile, pair_lds, ptap, wscale);
    else if (RS == 9)
        pair_pack_tile<9, PAIR_T>(d, tile, pair_lds, ptap, wscale);
    else if (RS == 1)
        pair_pack_tile<1, PAIR_T>(d, tile, pair_lds, ptap, wscale);
    else if (RS > 16)
        pair_pack_tile<0, 16>(d, tile, pair_lds, ptap, wscale);
    else
        pair_pack_tile<0, PAIR_T>(d, tile, pair_lds, ptap, wscale);
}

int amax_flat(const float *w, long n, float *q, hipStream_t st, int rs = 0, int taps = 0)
{
    AmaxTable t;
    memset(&t, 0, sizeof(t));
    t.w[0] = const_cast<float *>(w); t.q[0] = q; t.n[0] = n; t.rs[0] = (short)rs; t.taps[0] = (short)taps;
    hipLaunchKernelGGL(amax_multi_kernel, dim3(WQ_SLOTS, 1), dim3(256), 0, st, t);      // always all slots: images compare equal
    return 0;
}

}   // namespace

STEM_EXPORT size_t stem_f16x2_planes_qrec_offset(long npix, int C) { return C % 32 ? 0 : planes_payload(npix, C); }

STEM_EXPORT size_t stem_f16x2_planes_bytes(long npix, int C)
{
    return C % 32 ? 0 : planes_payload(npix, C) + (((QREC_HDR + planes_slots(npix, C)) * sizeof(float) + 15) & ~(size_t)15);
}

STEM_EXPORT size_t stem_f16x2_conv_weight_bytes(int C, int R, int S) { return C % 32 ? 0 : w_image_bytes(C, R, S) + WQ_BYTES; }

STEM_EXPORT size_t stem_f16x2_conv_weight_gen_bytes(int N, int C, int R, int S)
{
    return C % 32 ? 0 : gen_image_bytes(N, C, R, S) + WQ_BYTES;
}

STEM_EXPORT int stem_amax_nhwc(const float *x, int ldx, long npix, int C, float *q, long max_slots, void *stream)
{
    STEM_CHECK_ARG(x && q && npix >= 0 && C > 0 && C % 4 == 0 && ldx >= C && ldx % 4 == 0 && max_slots >= 1,
                   "stem_amax_nhwc: rows of C %% 4 == 0 floats, 16-byte aligned (C=%d ldx=%d)", C, ldx);
    long wg = (long)cdivz((size_t)npix * (C / 4), 2048);
    if (wg < 1) wg = 1;
    if (wg > max_slots) wg = max_slots;
    if (wg > 1024) wg = 1024;
    hipLaunchKernelGGL(amax_nhwc_kernel, dim3((unsigned)wg), dim3(256), 0, (hipStream_t)stream, x, ldx, npix, C / 4, q);
    STEM_LAUNCH_CHECK("stem_amax_nhwc");
    return 0;
}

// z: null for the plain split
static int split_nhwc(const float *x, int ldx, const float *z, int ldz, float slope, void *xp, float *xq, const float *src_q, long npix, int C,
                      void *stream, const char *who)
{
    const long np = npix * (C / 32) * 4;
    if (np == 0) return 0;
    if (!src_q && stem_amax_nhwc(x, ldx, npix, C, xq, planes_slots(npix, C), stream)) return -2;
    hipLaunchKernelGGL(z ? split_nhwc_kernel<true> : split_nhwc_kernel<false>, dim3((unsigned)cdivz(np, 256)), dim3(256), 0, (hipStream_t)stream,
                       x, ldx, z, ldz, slope, static_cast<unsigned char *>(xp), np, C / 32, xq, src_q ? src_q : xq);
    STEM_LAUNCH_CHECK(who);
    return 0;
}

STEM_EXPORT int stem_f16x2_split_nhwc(const float *x, int ldx, void *xp, float *xq, const float *src_q, long npix, int C, void *stream)
{
    STEM_CHECK_ARG(x && xp && xq && npix >= 0 && C > 0 && C % 32 == 0 && ldx >= C && ldx % 4 == 0,
                   "stem_f16x2_split_nhwc: channels must be a multiple of 32 and rows 16-byte aligned (C=%d ldx=%d)", C, ldx);
    return split_nhwc(x, ldx, nullptr, 0, 0.f, xp, xq, src_q, npix, C, stream, "stem_f16x2_split_nhwc");
}

STEM_EXPORT int stem_f16x2_split_dact_nhwc(const float *x, int ldx, const float *z, int ldz, float slope, void *xp, float *xq, const float *src_q,
                                            long npix, int C, void *stream)
{
    STEM_CHECK_ARG(x && z && xp && xq && npix >= 0 && C > 0 && C % 32 == 0 && ldx >= C && ldx % 4 == 0 && ldz >= C && ldz % 4 == 0,
                   "stem_f16x2_split_dact_nhwc: channels must be a multiple of 32 and rows 16-byte aligned (C=%d ldx=%d ldz=%d)", C, ldx, ldz);
    return split_nhwc(x, ldx, z, ldz, slope, xp, xq, src_q, npix, C, stream, "stem_f16x2_split_dact_nhwc");
}

STEM_EXPORT int stem_f16x2_merge_nhwc(const void *xp, const float *xq, float *x, int ldx, long npix, int C, void *stream)
{
    STEM_CHECK_ARG(x && xp && xq && npix >= 0 && C > 0 && C % 32 == 0 && ldx >= C, "stem_f16x2_merge_nhwc: bad arguments (C=%d ldx=%d)", C, ldx);
    const long ne = npix * C;
    if (ne == 0) return 0;
    hipLaunchKernelGGL(merge_planes_kernel, dim3((unsigned)cdivz(ne, 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned char *>(xp), x, ldx, ne, C, xq);
    STEM_LAUNCH_CHECK("stem_f16x2_merge_nhwc");
    return 0;
}

static int pack_conv_weight(const float *w, void *wp, int N, int C, int R, int S, int flip, void *stream, const char *who)
{
    STEM_CHECK_ARG(w && wp && N >= 1 && N <= BN && C > 0 && C % 32 == 0 && R >= 1 && S >= 1 && R * S <= MAXTAP,
                   "%s: N <= %d, C %% 32 == 0, R*S <= %d (N=%d C=%d R=%d S=%d)", who, BN, MAXTAP, N, C, R, S);
    const long np = (long)(C / 32) * R * S * BN * 4;
    float *wq = reinterpret_cast<float *>(static_cast<unsigned char *>(wp) + w_image_bytes(C, R, S));
    amax_flat(w, (long)N * C * R * S, wq, (hipStream_t)stream);
    hipLaunchKernelGGL(pack_weight_kernel<BN>, dim3((unsigned)cdivz(np, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       static_cast<unsigned char *>(wp), N, C, R * S, R * S, flip, np, wq);
    STEM_LAUNCH_CHECK(who);
    return 0;
}

STEM_EXPORT int stem_f16x2_pack_conv_weight(const float *w, void *wp, int N, int C, int R, int S, void *stream)
{
    return pack_conv_weight(w, wp, N, C, R, S, 0, stream, "stem_f16x2_pack_conv_weight");
}

STEM_EXPORT int stem_f16x2_pack_conv_weight_flip(const float *w, void *wp, int N, int C, int R, int S, void *stream)
{
    return pack_conv_weight(w, wp, N, C, R, S, 1, stream, "stem_f16x2_pack_conv_weight_flip");
}

STEM_EXPORT int stem_f16x2_pack_conv_weight_gen(const float *w, void *wp, int N, int C, int R, int S, int flip, int taps, void *stream)
{
    STEM_CHECK_ARG(w && wp && N >= 1 && C > 0 && C % 32 == 0 && R >= 1 && S >= 1 && R * S <= MAXTAP,
                   "stem_f16x2_pack_conv_weight_gen: C %% 32 == 0, R*S <= %d (N=%d C=%d R=%d S=%d)", MAXTAP, N, C, R, S);
    STEM_CHECK_ARG(taps >= 0 && taps <= R * S && (taps == 0 || !flip), "stem_f16x2_pack_conv_weight_gen: 0 <= taps <= R*S, forward role only (taps=%d)", taps);
    const int T = taps > 0 ? taps : R * S;
    const long np = (long)cdiv(N, GBN) * (C / 32) * T * GBN * 4;
    float *wq = reinterpret_cast<float *>(static_cast<unsigned char *>(wp) + gen_image_bytes(N, C, R, S));
    amax_flat(w, (long)N * C * R * S, wq, (hipStream_t)stream, R * S, taps < R * S ? taps : 0);
    hipLaunchKernelGGL(pack_weight_kernel<GBN>, dim3((unsigned)cdivz(np, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       static_cast<unsigned char *>(wp), N, C, R * S, T, flip, np, wq);
    STEM_LAUNCH_CHECK("stem_f16x2_pack_conv_weight_gen");
    return 0;
}

STEM_EXPORT int stem_f16x2_pack_conv_weights_multi(const stem_f16x2_pack_desc *descs_host, int n, void *stream)
{
    STEM_CHECK_ARG(descs_host && n >= 1 && n <= MAXPACK, "stem_f16x2_pack_conv_weights_multi: 1..%d descriptors per call, got %d", MAXPACK, n);
    size_t maxu = 0;
    for (int i = 0; i < n; ++i) {
        const stem_f16x2_pack_desc &d = descs_host[i];
        STEM_CHECK_ARG(d.w && d.wp && d.N >= 1 && d.C > 0 && d.C % 32 == 0 && d.R >= 1 && d.S >= 1 && d.R * d.S <= MAXTAP,
                       "stem_f16x2_pack_conv_weights_multi: descriptor %d: C %% 32 == 0, R*S <= %d (N=%d C=%d R=%d S=%d)", i, MAXTAP, d.N, d.C, d.R, d.S);
        const size_t nu = (size_t)cdiv(d.N, GBN) * (GBN / PKR) * (d.C / 32);
        if (nu > maxu) maxu = nu;
    }
    PackTable tab;
    memset(&tab, 0, sizeof(tab));
    memcpy(tab.d, descs_host, n * sizeof(stem_f16x2_pack_desc));
    AmaxTable mt;                           // max |w| of every tensor first: the scale its image is stored with
    memset(&mt, 0, sizeof(mt));
    for (int i = 0; i < n; ++i) {
        const stem_f16x2_pack_desc &d = descs_host[i];
        STEM_CHECK_ARG(d.taps >= 0 && d.taps <= d.R * d.S && (d.taps == 0 || !d.flip), "stem_f16x2_pack_conv_weights_multi: descriptor %d: taps", i);
        STEM_CHECK_ARG(d.flip >= 0 && d.flip <= 2 && (d.flip != 2 || (d.R == d.S && (d.R & 1))),
                       "stem_f16x2_pack_conv_weights_multi: descriptor %d: flip 0 | 1 | 2 (2 = phase images of a transposed face: odd square windows)", i);
        mt.w[i] = static_cast<float *>(const_cast<void *>(d.w));
        mt.q[i] = reinterpret_cast<float *>(static_cast<unsigned char *>(d.wp) + gen_image_bytes(d.N, d.C, d.R, d.S));
        mt.n[i] = (long)d.N * d.C * d.R * d.S;
        mt.rs[i] = (short)(d.R * d.S);
        mt.taps[i] = (short)(d.taps > 0 && d.taps < d.R * d.S ? d.taps : 0);
    }
    bool all_bmax = true;
    for (int i = 0; i < n; ++i) all_bmax = all_bmax && descs_host[i].bmax != nullptr && descs_host[i].nb >= 1;
    if (!all_bmax) {
        for (int i = 0; i < n; ++i) tab.d[i].bmax = nullptr;        // one source of the maximum per call
        hipLaunchKernelGGL(amax_multi_kernel, dim3(WQ_SLOTS, n), dim3(256), 0, (hipStream_t)stream, mt);
    }
    const unsigned gx = (unsigned)(maxu < 2048 ? maxu : 2048);
    hipLaunchKernelGGL(pack_weight_gen_multi_kernel, dim3(gx, n), dim3(256), 0, (hipStream_t)stream, tab);
    STEM_LAUNCH_CHECK("stem_f16x2_pack_conv_weights_multi");
    return 0;
}

/* Both images of every layer from one read of its weights (csrc: pack_weight_pair_multi_kernel): descs[i] names the torch tensor
 * [A][B][R][S], up to two images (role 0 / 1: destination, rows = a or b, tap order, live-tap prefix) and the optimiser pass's
 * chunk maxima that cover it (mandatory here: the launch has no maximum pass of its own).  Images of a layer whose row count is
 * not a multiple of 128 must have been zero-filled once (the padding rows are never written).  What it replaces:
 * stem_f16x2_pack_conv_weights_multi called once per role after every optimiser step (stem/trainSTEM.py:213). */
STEM_EXPORT int stem_f16x2_pack_conv_weights_pair_multi(const stem_f16x2_pair_desc *descs, int n, void *stream)
{
    STEM_CHECK_ARG(descs && n >= 1 && n <= MAXPAIR, "stem_f16x2_pack_conv_weights_pair_multi: 1..%d descriptors per call, got %d", MAXPAIR, n);
    PairTable tab;
    memset(&tab, 0, sizeof(tab));
    int tiles = 0;
    size_t lds = 0;
    for (int i = 0; i < n; ++i) {
        const stem_f16x2_pair_desc &h = descs[i];
        STEM_CHECK_ARG(h.w && h.A >= 1 && h.B >= 1 && h.R >= 1 && h.S >= 1 && h.R * h.S <= MAXTAP && h.bmax && h.nb >= 1,
                       "stem_f16x2_pack_conv_weights_pair_multi: descriptor %d: tensor, window (<= %d taps) and chunk maxima are mandatory", i, MAXTAP);
        PairDesc &d = tab.d[i];
        d.w = static_cast<float *>(const_cast<void *>(h.w));
        d.A = h.A; d.B = h.B; d.R = h.R; d.S = h.S; d.bmax = h.bmax; d.b0 = h.b0; d.nb = h.nb;
        const void *wps[2] = {h.wp0, h.wp1};
        const int modes[2] = {h.mode0, h.mode1}, taps[2] = {h.taps0, h.taps1};
        for (int r = 0; r < 2; ++r) {
            d.role[r].wp = const_cast<void *>(wps[r]);
            if (!wps[r]) continue;
            d.role[r].rows_b = modes[r] & 1;
            d.role[r].tapmode = modes[r] >> 1;
            d.role[r].taps = taps[r];
            const int C = d.role[r].rows_b ? h.A : h.B;
            STEM_CHECK_ARG(d.role[r].tapmode >= 0 && d.role[r].tapmode <= 2 && C % 32 == 0 && taps[r] >= 0 && taps[r] <= h.R * h.S &&
                           (taps[r] == 0 || (d.role[r].tapmode == 0 && r == 0)) && (d.role[r].tapmode != 2 || (h.R == h.S && (h.R & 1))),
                           "stem_f16x2_pack_conv_weights_pair_multi: descriptor %d role %d: contraction channels %% 32, tap order 0..2, a live-tap "
                           "prefix only for role 0 in identity order, phase order for odd square windows", i, r);
        }
        d.tile0 = tiles;
        tiles += cdiv(h.A, pair_ta(h.R * h.S)) * cdiv(h.B, PAIR_T);
        const size_t need = (size_t)pair_ta(h.R * h.S) * (PAIR_T * h.R * h.S + PAIR_PAD) * sizeof(float) + 32 * sizeof(int);
        if (need > lds) lds = need;
    }
    tab.n = n;
    static size_t attr_lds = 0;
    if (lds > attr_lds) {
        (void)hipFuncSetAttribute((const void *)pack_weight_pair_multi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_lds = lds;
    }
    hipLaunchKernelGGL(pack_weight_pair_multi_kernel, dim3(tiles), dim3(PAIR_NT), lds, (hipStream_t)stream, tab);
    STEM_LAUNCH_CHECK("stem_f16x2_pack_conv_weights_pair_multi");
    return 0;
}
