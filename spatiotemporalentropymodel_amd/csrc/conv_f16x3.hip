// fp32-accurate convolutions on the fp16 matrix cores of gfx950 (MI355X): the FROZEN analysis transform (first part of this
// file) and the general kernel for the training-time STEM layers (second part); weight gradients: wgrad_f16x3.hip.
//
// v_mfma_f32_32x32x2_f32 (igemm.hip) is the only MFMA that multiplies fp32 operands, at 64 flop/clk/SIMD; the 16-bit forms
// (v_mfma_f32_32x32x16_f16 / _bf16) run at 1024.  With every fp32 number stored as two fp16 numbers of a scaled copy (stem_common.h:
// "the 16-bit operands") three fp16 MFMAs (K = 16 each, 32 cycles) replace eight fp32 MFMAs (K = 2 each, 64 cycles): 96 instead
// of 512 matrix-pipe cycles per 16 input channels, with fp32 accumulation throughout (tests: the 1e-4 gates of the fp32 path;
// measured 1-2.5e-6 of max|ref| per layer, the fp32-MFMA kernels' own distance from fp64).  Round 2 used three bf16 planes and
// six products (no scaling needed, twice the MFMAs).  A convolution epilogue takes the scale of its planes output from the bound
// K max|x| max|w| + max|bias| (one layer's worth of over-estimate: the inputs' maxima are measured).
//
// Operands: planes tensors and packed weight images as f16x3_layout.h states them, produced by the epilogues here and by
// f16x3_pack.hip; the weights of the analysis transform are frozen (stem/trainSTEM.py:128) and packed once.
//
// Tile: 128 pixels x 192 channels per workgroup, 8 wavefronts as 4 (M) x 2 (N), each 32 x 96 = three 32x32 accumulators;
// K chunk = one tap x 32 input channels = 2 k-steps x 3 tiles x 3 products = 18 MFMAs per wavefront.  LDS rows are 64 B
// (32 fp16) per plane with the 16-byte piece index XOR-swizzled by (row >> 2) & 3: ds_read_b128 is conflict-free without
// padding.  The ring is filled by LDS-DMA (global -> LDS, no vector registers; "LDS-DMA" below): the packed weight chunk IS the
// LDS image and is copied linearly, an activation row's swizzle is applied on the source side (the lane at LDS slot s fetches piece
// s ^ ((row >> 2) & 3) of its pixel), taps outside the image and rows beyond M read as zeros through an offset the buffer view
// rejects.  With three LDS stages (DEPTH 3) a copy has two chunks' time to land: the step of chunk c reads the second k-step of
// chunk c, waits (counted vmcnt: all but the youngest chunk's copies) and meets the barrier in its middle, then issues the copy
// of chunk c + 3 into the stage chunk c released, between the MFMAs of its second half, which also carry the reads of chunk
// c + 1's first k-step.  With two stages (DEPTH 2, and the general kernel below) the copy of chunk c + 1 is issued at the top of
// chunk c and has landed at the barrier that ends it.  Every reuse of the ring behind the loop waits for the copies still in flight.
// The same products are also instantiated on v_mfma_f32_16x16x32_f16 (MS 16: one k-step per chunk, twice the instructions of
// half the size, a permuted accumulator layout that keeps ds_read_b128 conflict-free on the same LDS image): equal or slower
// alone, faster on a loaded, power-limited chip -- which is where these kernels run.
// The GDN that follows every analysis convolution (gdn.py:52-67) is fused: second contraction over the squared outputs, which
// are scaled by the tile's own maximum, split and parked in LDS as A-operand images; gamma' streams in as a packed 1x1 weight
// image; the same fp16 instruction.
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "f16x3_tail.h"

namespace {

constexpr int XP = BN + 4;                                        // fp32 pitch of the tile parked for the planes pass
// LDS of a BM-pixel tile: the largest of the main loop (2 x NPL planes x (BM + BN) rows x 64 B), the fused GDN (the squares of six
// 32-channel slabs as A-operand images + one chunk of gamma') and the planes pass (BM x XP floats); then the tap table
constexpr int imax(int a, int b) { return a > b ? a : b; }
constexpr int lds_stages(int depth) { return depth == 3 ? 3 : 2; }
constexpr int lds_taps(int bm, int depth) { return imax(imax(lds_stages(depth) * NPL * (bm + BN) * 64, 6 * NPL * bm * 64 + NPL * BN * 64), bm * XP * 4); }
constexpr int lds_total(int bm, int depth) { return lds_taps(bm, depth) + 32 * 4; }

struct Fx3Phase {
    int ntaps, S;                  // taps of this phase's window (row-major, S per row)
    int dy0, dx0;                  // offset of its first tap on the coarse grid; tap t reads (qy + dy0 + t / S, qx + dx0 + t % S)
    int wofs;                      // byte offset of its weight image inside wp
    int cps, nsplit;               // split-K plan of this phase (blocks with blockIdx.z >= nsplit leave at once)
    int wsofs;                     // float offset of its partial-tile slabs inside ws
    int ooy, oox;                  // py, px
};

struct Fx3Args {
    const void *xp, *wp;
    const float *xq, *wq;          // scale records of the two operands (stem_common.h)
    float *yq;                     // ... of the output: slots always, the scale when planes are written (may be null without planes)
    const float *bias, *beta;
    const void *gp;                // fused GDN: gamma' as the packed weight image of a 1x1 convolution (N x ceil32(N)), its record behind it
    const float *gq;
    float *y;
    void *yp;
    int ldy;
    int B, H, W, C, N, OH, OW, stride, ntaps;
    int S;                         // taps per filter row: tap t = (t / S, t % S) of the R x S window (ntaps may be a prefix)
    int xbytes, wbytes, gbytes;
    float beta_bound;
    int fuse;                      // 0: bias only, 1: GDN
    // general variant (conv_f16x3_gen_kernel): activation epilogue, N tiles, split-K
    const float *z;                // EPI_DACT: the activation output the slope is selected by (z > 0 ? 1 : slope)
    int ldz, epi;                  // epi: 0 bias, 1 bias + leaky ReLU, 2 times d(leaky ReLU)(z)
    float slope;
    float *ws;                     // split-K partial tiles [nsplit][M][gridDim.y * BN]
    int *cnt;                      // one arrival counter per output tile, zero before and after every launch
    int nsplit, cps;               // blockIdx.z = split, chunks [split * cps, (split + 1) * cps)
    int xpix;                      // bytes per pixel of the planes buffer x lives in (a 32-channel-aligned slice of a wider tensor)
    signed char dy[MAXTAP], dx[MAXTAP];
    // transposed face of a stride-2 layer as ONE launch over its four sub-pixel phases (conv_f16x3_gen_kernel<.., .., true>):
    // blockIdx.x = phase * ptiles + pixel tile of the COARSE grid (OH x OW = H x W here); phase (py, px) is a stride-1 convolution
    // of the coarse grid with its own regular window of taps and weight image, written to the fine pixels (2 qy + py, 2 qx + px)
    // of the OHf x OWf output
    int ptiles, btaps, OHf, OWf;   // btaps: the tap count of the output bound (the largest phase's: one scale for all phases)
    Fx3Phase ph[4];
};

// Byte offset of tap t = (t / S, t % S) relative to a pixel's own position in the planes.  The kernels walk it in scalar
// registers (TAP_WALK_NEXT): a table lookup in LDS would drain the wavefront's LDS queue in the middle of the woven block.
#define TAP_OFFSET(t) (tw_first + ((t) / tw_S) * tw_line + ((t) % tw_S) * tw_col)
#define TAP_WALK_NEXT()                                                                         \
    do {                                                                                        \
        const bool wrap_ = pf_t + 1 == tw_T, rowend_ = pf_ts + 1 == tw_S;                       \
        ++pf_q;                                                                                 \
        pf_to = wrap_ ? tw_first : pf_to + (rowend_ ? tw_line - (tw_S - 1) * tw_col : tw_col);  \
        pf_ts = (wrap_ || rowend_) ? 0 : pf_ts + 1;                                             \
        pf_t = wrap_ ? 0 : pf_t + 1;                                                            \
        pf_kc += wrap_ ? 1 : 0;                                                                 \
    } while (0)


// BM = pixels per workgroup: 128 (8 wavefronts) or 64 (4 wavefronts, for layers with too few 128-pixel tiles to fill the chip).
// DEPTH 2: two LDS stages, the copy of chunk c + 1 in flight while chunk c is multiplied; the fragments of a 16-channel step are
//          read right before its MFMAs.
// DEPTH 3: three LDS stages -- chunks c + 1 (landed) and c + 2 (in flight) are in the ring while chunk c is multiplied, and the
//          copy of chunk c + 3 is issued in the second half of chunk c's step; the fragments of the NEXT 16-channel step (the first
//          one of chunk c + 1 included) are read between the MFMAs of the current one; only the wait and the barrier are left
//          between the two halves.  120 KB of LDS with 128-pixel tiles (one workgroup per CU either way).
// MS = rows of the MFMA shape: 32 (v_mfma_f32_32x32x16_f16) or 16 (v_mfma_f32_16x16x32_f16, three-stage loop only): the same
//      operands, LDS traffic and flop in twice as many instructions of half the size, which the chip runs at a higher clock where a
//      launch fills it and sits at the power limit (g_a.2: -6 %); smaller launches lose with it (more issue slots), so it is a
//      second instantiation.  MFMA row (column) m of a 16-block reads image row 4 PI[m >> 2] + (m & 3), PI = 0,2,3,1 -- with the
//      64-byte-row image and its XOR swizzle that makes the 16-lane groups of ds_read_b128 conflict-free -- so lane l holds
//      channels 16 nj + 4 PI[(l & 15) >> 2] + (l & 3) and pixel rows 16 mi + 4 PI[l >> 4] + i of the wavefront's 32 x 96 tile.
__device__ inline int pi4(int x) { return (0x78 >> (2 * x)) & 3; }

// LDS-DMA: the ring of both kernels is filled global -> LDS without a pass through the vector registers.  One instruction
// copies 1 KiB per wavefront: lane l's 16 bytes at (voff, soff) of the buffer view land at LDS byte lds_base + 16 l; an offset
// the view rejects (OOR) lands as zeros.  Issued as inline assembly, as in wgrad_f16x3.hip: the compiler orders every LDS read
// after ALL pending LDS-DMA it knows of, which would collapse the look-ahead; the ring is kept consistent by counted
// s_waitcnt vmcnt + barrier instead (LDS-DMA retires in issue order).  Vector-memory instructions of the compiler's own that
// are still pending only make a counted wait stricter.  M0 is reserved (not allocatable, not declarable as a clobber); these
// kernels have no other user of it.
typedef int rsrc4 __attribute__((ext_vector_type(4)));
__device__ inline rsrc4 dma_rsrc(const void *p, int bytes)
{
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    return rsrc4{(int)(unsigned)v, (int)(unsigned)(v >> 32), bytes, 0x00020000};
}
__device__ inline void dma16(const rsrc4 r, unsigned lds_base, int voff, int soff)
{
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_base), "v"(voff), "s"(r), "s"(soff) : "memory");
}
#define DMA_WAIT_BARRIER(n) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(n) : "memory")
// every LDS read of this wavefront has returned: as a builtin between two scheduling fences, so that the compiler's own
// wait-count pass knows it (conv_f16x3_img.hip)
#define LDS_READS_DONE()                            \
    do {                                            \
        __builtin_amdgcn_sched_barrier(0);          \
        __builtin_amdgcn_s_waitcnt(0xC07F);         \
        __builtin_amdgcn_sched_barrier(0);          \
    } while (0)

template <int BM, int DEPTH, int MS>
__global__ __launch_bounds__(BM * 4) void conv_f16x3_kernel(const Fx3Args a)
{
    static_assert(DEPTH == 2 || DEPTH == 3, "two or three LDS stages");
    static_assert(MS == 32 || (MS == 16 && DEPTH == 3), "the 16-row MFMA shape exists for the three-stage loop");
    constexpr int NT = BM * 4;
    constexpr int A_PLANE = BM * 64, A_BUF = NPL * A_PLANE;
    constexpr int PL = NPL;
    constexpr int WPIECES = PL * BN * 4;                // 16-byte pieces of the weight chunk
    static_assert(WPIECES % NT == 0, "every wavefront copies whole 1 KiB pieces of the weight chunk");
    constexpr int BP = WPIECES / NT;                    // ... per thread = LDS-DMA instructions per wavefront
    constexpr int NI = PL + BP;                         // LDS-DMA instructions per wavefront and chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NST = lds_stages(DEPTH);
    unsigned char *As = smem;                       // [NST][NPL][BM][64 B]
    unsigned char *Bs = smem + NST * A_BUF;         // [NST][NPL][BN][64 B]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Mtot = a.B * a.OH * a.OW;
    int tile_m = blockIdx.x;
    {   // XCD-aware tile order (see igemm.hip): neighbouring pixel tiles share one L2
        const int nb = gridDim.x, qq = nb >> 3, rr = nb & 7, xcd = tile_m & 7, idx = tile_m >> 3;
        if (nb >= 16) tile_m = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
    }
    const int bm0 = tile_m * BM;
    const int nslab = a.C / KC, pixbytes = nslab * SLAB;

    // ---- staging assignment.  Activations: thread -> (row = tid / 4, 16-byte LDS slot = tid % 4) of both planes: wavefront w's
    // 1 KiB of a plane is rows 16 w .. 16 w + 15, lane-linear.  The image's XOR swizzle permutes the pieces inside a row, so the
    // lane at slot s fetches piece s ^ ((row >> 2) & 3) of its pixel ------------------------------------------------------------
    const int srow = tid >> 2, scol = (tid & 3) ^ ((srow >> 2) & 3);
    int pb;
    unsigned pmask = 0;
    {
        const int m = bm0 + srow;
        const bool ok = m < Mtot;
        const int mm = ok ? m : 0;
        const int ohw = a.OH * a.OW, b = mm / ohw, rem = mm - b * ohw, qy = rem / a.OW, qx = rem - qy * a.OW;
        const int by = qy * a.stride, bx = qx * a.stride;
        pb = ((b * a.H + by) * a.W + bx) * pixbytes + scol * 16;
        for (int t = 0; t < a.ntaps; ++t) {
            const int iy = by + a.dy[t], ix = bx + a.dx[t];
            if (ok && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) pmask |= 1u << t;
        }
    }
    // weights: the chunk image is copied linearly, pass j = bytes [j NT 16, (j + 1) NT 16), wavefront w its 1 KiB of each pass
    const int wv0 = tid * 16;
    const int nchunks = a.ntaps * nslab;
    const int q_last = nchunks - 1;
    __syncthreads();

    const rsrc4 rx = dma_rsrc(a.xp, a.xbytes), rw = dma_rsrc(a.wp, a.wbytes);
    const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char *)smem;
    const unsigned ldsw = __builtin_amdgcn_readfirstlane(lds0 + wave * 1024);       // this wavefront's 1 KiB inside a piece group
    // chunk q = (tap t at byte offset tA, slab kc) -> LDS stage `stage`: NI instructions per wavefront, the planes first;
    // dma_range issues instructions [lo, hi) of them
    auto dma_range = [&](int stage, int t, int tA, int kc, int q, int lo, int hi) {
        const int sA = kc * SLAB, sB = q * B_BUF;
        const int mk = __builtin_amdgcn_sbfe((int)pmask, (unsigned)t, 1u);                 // 0 / -1: tap t inside the image
        const int off = ((pb + tA) & mk) | (OOR & ~mk);
        const unsigned la = ldsw + stage * A_BUF, lb = ldsw + NST * A_BUF + stage * B_BUF;
#pragma unroll
        for (int i = lo; i < hi; ++i) {
            if (i < PL)
                dma16(rx, la + i * A_PLANE, off + i * 64, sA);
            else
                dma16(rw, lb + (i - PL) * (NT * 16), wv0 + (i - PL) * (NT * 16), sB);
        }
    };
    auto dma = [&](int stage, int t, int tA, int kc, int q) { dma_range(stage, t, tA, kc, q, 0, NI); };

    // ---- wave tile -----------------------------------------------------------------------------------------------------
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 96;
    const int lr = lane & 31, lh = lane >> 5;
    const int sw = (lr >> 2) & 3;                                   // (row >> 2) & 3 of every row this lane reads
    const int rdA = (wm0 + lr) * 64, rdB = (wn0 + lr) * 64;
    const int pk0 = ((0 + lh) ^ sw) << 4, pk1 = ((2 + lh) ^ sw) << 4;
    // MS == 16 (see the kernel's header)
    const int l16 = lane & 15, lq = lane >> 4;
    const int cm = 4 * pi4(l16 >> 2) + (l16 & 3), rq = 4 * pi4(lq);
    const int rdA16 = (wm0 + cm) * 64 + ((lq ^ pi4(l16 >> 2)) << 4), rdB16 = (wn0 + cm) * 64 + ((lq ^ pi4(l16 >> 2)) << 4);
    // element (j, r) of this lane's accumulators: local pixel row / local channel inside the workgroup's tile
    auto ROWL = [&](int r) { return MS == 32 ? wm0 + (r & 3) + 8 * (r >> 2) + 4 * lh : wm0 + ((r >> 2) & 1) * 16 + rq + (r & 3); };
    auto COLL = [&](int j, int r) { return MS == 32 ? wn0 + j * 32 + lr : wn0 + j * 32 + (r >> 3) * 16 + cm; };
    f32x16 acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    // prefetch target of the next step (wave-uniform).  The byte offset of tap t inside the planes is carried along in scalar
    // registers (pf_ts = t % S): a table lookup in LDS would drain the wavefront's LDS queue in the middle of the woven block.
    int pf_q = 0, pf_t = 0, pf_kc = 0, pf_ts = 0, pf_to = 0;
    const int tw_T = a.ntaps, tw_S = a.S, tw_col = pixbytes, tw_line = a.W * pixbytes, tw_first = (a.dy[0] * a.W + a.dx[0]) * pixbytes;
    // DEPTH 2: chunk c + 1 is copied into the other stage (free since the barrier that ended chunk c - 1) while chunk c is
    // multiplied; it has landed, for every wavefront, behind the wait and the barrier that end the step
    auto step = [&](int cur) {
        const unsigned char *Ab = As + cur * A_BUF + rdA, *Bb = Bs + cur * B_BUF + rdB;
        const int t = __builtin_amdgcn_readfirstlane(pf_t), kc = __builtin_amdgcn_readfirstlane(pf_kc), q = __builtin_amdgcn_readfirstlane(pf_q);
        const int to = __builtin_amdgcn_readfirstlane(pf_to);
        dma(cur ^ 1, t, to, kc, q);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pk = ks ? pk1 : pk0;
            h16x8 af[PL], bf[PL][3];
#pragma unroll
            for (int pl = 0; pl < PL; ++pl) af[pl] = *reinterpret_cast<const h16x8 *>(Ab + pl * A_PLANE + pk);
#pragma unroll
            for (int pl = 0; pl < PL; ++pl)
#pragma unroll
                for (int j = 0; j < 3; ++j) bf[pl][j] = *reinterpret_cast<const h16x8 *>(Bb + pl * B_PLANE + j * 32 * 64 + pk);
#pragma unroll
            for (int j = 0; j < 3; ++j) {      // smallest terms first
                acc[j] = STEM_MFMA16(af[1], bf[0][j], acc[j]);
                acc[j] = STEM_MFMA16(af[0], bf[1][j], acc[j]);
                acc[j] = STEM_MFMA16(af[0], bf[0][j], acc[j]);
            }
        }
        if (pf_q < q_last) TAP_WALK_NEXT();
        DMA_WAIT_BARRIER(0);
    };
    // DEPTH 3: F0 holds the fragments of (stage rd, channels 0..15) on entry and of (stage nx, channels 0..15) on exit
    h16x8 f0a[PL], f0b[PL][3], f1a[PL], f1b[PL][3];
    auto lfrag = [&](int stage, int pk, h16x8 (&af)[PL], h16x8 (&bf)[PL][3]) {       // in the order the MFMAs consume them
        const unsigned char *Ab = As + stage * A_BUF + rdA + pk, *Bb = Bs + stage * B_BUF + rdB + pk;
        af[1] = *reinterpret_cast<const h16x8 *>(Ab + A_PLANE);
        bf[0][0] = *reinterpret_cast<const h16x8 *>(Bb);
        af[0] = *reinterpret_cast<const h16x8 *>(Ab);
        bf[1][0] = *reinterpret_cast<const h16x8 *>(Bb + B_PLANE);
#pragma unroll
        for (int j = 1; j < 3; ++j) {
            bf[0][j] = *reinterpret_cast<const h16x8 *>(Bb + j * 32 * 64);
            bf[1][j] = *reinterpret_cast<const h16x8 *>(Bb + B_PLANE + j * 32 * 64);
        }
    };
    auto mfma9 = [&](h16x8 (&af)[PL], h16x8 (&bf)[PL][3]) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            acc[j] = STEM_MFMA16(af[1], bf[0][j], acc[j]);
            acc[j] = STEM_MFMA16(af[0], bf[1][j], acc[j]);
            acc[j] = STEM_MFMA16(af[0], bf[0][j], acc[j]);
        }
    };
    // The three stages hold chunks c (rd), c + 1 (nx) and c + 2 (in flight).  The step of chunk c:
    //   X: MFMAs (c, 0)  +  reads (c, 1)
    //      wait: this wavefront's reads of chunk c are done, its share of chunk c + 1 has landed (all but the youngest chunk's
    //      NI instructions); barrier: everybody's
    //   Y: copy of chunk c + 3 into the stage chunk c has just released, MFMAs (c, 1)  +  reads (c + 1, 0)
    // so a copy has two chunks' time to land.  Beyond the last chunk the copy re-fetches the last chunk into a free stage and the
    // look-ahead reads fetch fragments nobody multiplies: vmcnt(NI) always means "everything but the youngest chunk".
    auto step3 = [&](int rd, int nx) {
        const int t = __builtin_amdgcn_readfirstlane(pf_t), kc = __builtin_amdgcn_readfirstlane(pf_kc), q = __builtin_amdgcn_readfirstlane(pf_q);
        const int to = __builtin_amdgcn_readfirstlane(pf_to);
        lfrag(rd, pk1, f1a, f1b);
        mfma9(f0a, f0b);
        // issue order: one LDS read behind each of the first eight MFMAs
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        LDS_READS_DONE();
        DMA_WAIT_BARRIER(NI);
        // Y: one of the copy's NI <= 8 instructions and one read in front of each of the first eight MFMAs -- every wavefront leaves
        // the barrier at the same moment, and NI copies in a row from each of them would queue in front of the MFMAs
        static_assert(NI <= 8, "one copy instruction per MFMA of the second half");
        const unsigned char *Ab = As + nx * A_BUF + rdA + pk0, *Bb = Bs + nx * B_BUF + rdB + pk0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int j = i / 3, k = i % 3;            // mfma9's order
            if (i < NI) dma_range(rd, t, to, kc, q, i, i + 1);
            if (i == 0) f0a[1] = *reinterpret_cast<const h16x8 *>(Ab + A_PLANE);        // lfrag's order
            if (i == 1) f0b[0][0] = *reinterpret_cast<const h16x8 *>(Bb);
            if (i == 2) f0a[0] = *reinterpret_cast<const h16x8 *>(Ab);
            if (i == 3) f0b[1][0] = *reinterpret_cast<const h16x8 *>(Bb + B_PLANE);
            if (i >= 4 && i < 8) f0b[i & 1][(i - 2) >> 1] = *reinterpret_cast<const h16x8 *>(Bb + (i & 1) * B_PLANE + ((i - 2) >> 1) * 32 * 64);
            acc[j] = STEM_MFMA16(k == 0 ? f1a[1] : f1a[0], k == 1 ? f1b[1][j] : f1b[0][j], acc[j]);
            if (i < 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
        LDS_READS_DONE();          // said here, so that the wait-count pass does not drain the NEXT step's reads in front of its MFMAs
        if (pf_q < q_last) TAP_WALK_NEXT();
    };

    // MS == 16: a chunk is ONE k-step of the 16x16x32 instruction; its two halves are the channel blocks 0..2 / 3..5 of the
    // wavefront's 96 columns.  ga[s] = pixel fragments of the chunk in flight (two sets: the next chunk's are read during the
    // second half), gb0 / gb1 = weight fragments of the two halves.
    h16x8 ga[2][2][PL], gb0[3][PL], gb1[3][PL];
    f32x4 a16[2][6];
    if constexpr (MS == 16) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int nj = 0; nj < 6; ++nj) a16[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    auto lfragA16 = [&](const unsigned char *base, h16x8 (&A)[2][PL]) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int pl = 0; pl < PL; ++pl) A[mi][pl] = *reinterpret_cast<const h16x8 *>(base + rdA16 + mi * 16 * 64 + pl * A_PLANE);
    };
    auto lfragB16 = [&](const unsigned char *base, int half, h16x8 (&B)[3][PL]) {
#pragma unroll
        for (int n3 = 0; n3 < 3; ++n3)
#pragma unroll
            for (int pl = 0; pl < PL; ++pl) B[n3][pl] = *reinterpret_cast<const h16x8 *>(base + rdB16 + (half * 3 + n3) * 16 * 64 + pl * B_PLANE);
    };
    auto mma18 = [&](h16x8 (&A)[2][PL], h16x8 (&B)[3][PL], int half, f32x4 (&d)[2][6]) {
        // smallest terms first; the six accumulators of a product follow each other (independent instructions back to back)
#pragma unroll
        for (int prod = 0; prod < 3; ++prod)
#pragma unroll
            for (int n3 = 0; n3 < 3; ++n3)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    d[mi][half * 3 + n3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[mi][prod == 0 ? 1 : 0], B[n3][prod == 1 ? 1 : 0],
                                                                                   d[mi][half * 3 + n3], 0, 0, 0);
    };
    // the X / wait + barrier / Y form of step3: X = first half's 18 MFMAs + the 6 reads of the second half's weights, Y = the copy
    // of chunk c + 3, the second half's 18 MFMAs + the 10 reads of chunk c + 1's pixels and first-half weights
    auto step3_16 = [&](int rd, int nx, h16x8 (&Acur)[2][PL], h16x8 (&Anext)[2][PL]) {
        const int t = __builtin_amdgcn_readfirstlane(pf_t), kc = __builtin_amdgcn_readfirstlane(pf_kc), q = __builtin_amdgcn_readfirstlane(pf_q);
        const int to = __builtin_amdgcn_readfirstlane(pf_to);
        lfragB16(Bs + rd * B_BUF, 1, gb1);
        mma18(Acur, gb0, 0, a16);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
        LDS_READS_DONE();
        DMA_WAIT_BARRIER(NI);
        // Y in five groups of (a share of the copy's instructions, 3 / 3 / 2 / 2 / 0 reads, 4 or 3 MFMAs): every wavefront leaves
        // the barrier at the same moment, and NI copies in a row from each of them would queue in front of the MFMAs
        auto ygroup = [&](auto group_tag) {
            constexpr int g = decltype(group_tag)::value;
            constexpr int r0 = g < 2 ? 3 * g : g < 4 ? 2 * g + 2 : 10, r1 = g < 1 ? 3 : g < 3 ? 2 * g + 4 : 10;
            constexpr int m0 = (g * 18 + 4) / 5, m1 = ((g + 1) * 18 + 4) / 5;
            dma_range(rd, t, to, kc, q, (g * NI + 4) / 5, ((g + 1) * NI + 4) / 5);
#pragma unroll
            for (int r = r0; r < r1; ++r) {                                         // lfragA16's, then lfragB16's order
                if (r < 4)
                    Anext[r >> 1][r & 1] = *reinterpret_cast<const h16x8 *>(As + nx * A_BUF + rdA16 + (r >> 1) * 16 * 64 + (r & 1) * A_PLANE);
                else
                    gb0[(r - 4) >> 1][r & 1] = *reinterpret_cast<const h16x8 *>(Bs + nx * B_BUF + rdB16 + ((r - 4) >> 1) * 16 * 64 + (r & 1) * B_PLANE);
            }
#pragma unroll
            for (int m = m0; m < m1; ++m) {                                         // mma18's order: product, channel block, pixel block
                const int prod = m / 6, n3 = (m % 6) >> 1, mi = m & 1;
                a16[mi][3 + n3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Acur[mi][prod == 0 ? 1 : 0], gb1[n3][prod == 1 ? 1 : 0], a16[mi][3 + n3], 0, 0, 0);
            }
            if constexpr (r1 > r0) __builtin_amdgcn_sched_group_barrier(0x100, r1 - r0, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, m1 - m0, 0);
        };
        ygroup(std::integral_constant<int, 0>{});
        ygroup(std::integral_constant<int, 1>{});
        ygroup(std::integral_constant<int, 2>{});
        ygroup(std::integral_constant<int, 3>{});
        ygroup(std::integral_constant<int, 4>{});
        LDS_READS_DONE();
        if (pf_q < q_last) TAP_WALK_NEXT();
    };

    // chunk q = kc * ntaps + t (channel slab outer, taps inner: the taps of one slab re-touch the same input lines)
    auto chunk_of = [&](int q, int &t, int &kc) {
        q = q < q_last ? q : q_last;
        kc = q / a.ntaps;
        t = q - kc * a.ntaps;
        return q;
    };
    {
        int t, kc, q;
        constexpr int PRE = DEPTH == 3 ? 3 : 1;    // chunks on their way to stages 0 .. PRE - 1 before the loop starts
#pragma unroll
        for (int c = 0; c < PRE; ++c) {
            q = chunk_of(c, t, kc);
            dma(c, t, TAP_OFFSET(t), kc, q);
        }
        pf_q = chunk_of(PRE, pf_t, pf_kc);
        pf_ts = pf_t % tw_S;
        pf_to = TAP_OFFSET(pf_t);
    }
    // ---- scales of the epilogue, computed HERE: their slot / bias / beta loads and block reductions run while the first chunks
    // are in flight instead of after the last MFMA (one workgroup per CU: nothing else would hide them there)
    __shared__ float qred[16];
    const float fac = q_inv(a.xq) * q_inv(a.wq);                   // the operands were stored times 2^ex, 2^ew
    float oscale = 1.f;                                            // 2^e of the planes output
    if (a.yp) {
        // tail_oscale's bound (f16x3_tail.h) times the fused GDN's factor (GDN divides by at least sqrt(min beta')), written out
        // here: every factoring of it that was tried cost one of the six instantiations 1 to 4 vector registers.
        const float xmax = q_amax(a.xq, qred), wmax = q_amax(a.wq, qred);
        float bm = 0.f, btm = 3.0e38f;
        for (int n = tid; n < a.N; n += NT) {
            if (a.bias) bm = fmaxf(bm, fabsf(a.bias[n]));
            if (a.fuse) {
                const float bb = fmaxf(a.beta[n], a.beta_bound);
                btm = fminf(btm, bb * bb - 1.4551915228366852e-11f);
            }
        }
        bm = block_max(bm, qred);
        float ob = (float)(a.C * a.ntaps) * xmax * wmax + bm;
        if (a.fuse) ob *= __builtin_amdgcn_rsqf(fmaxf(-block_max(-btm, qred), 1e-30f));
        const int oe = q_exp(ob);
        oscale = q_pow2(oe);
        if (blockIdx.x == 0 && tid == 0) a.yq[1] = q_pow2(-oe);
    }
    // chunk 0 has landed: this wavefront's share (everything but the two younger chunks of the three-stage ring), then everybody's
    __syncthreads();
    DMA_WAIT_BARRIER(DEPTH == 3 ? 2 * NI : 0);
    if constexpr (MS == 16) {
        int rd = 0, nx = 1, wr = 2;
        lfragA16(As, ga[0]);
        lfragB16(Bs, 0, gb0);
        LDS_READS_DONE();
        int q = 0;
        for (; q + 1 < nchunks; q += 2) {
            step3_16(rd, nx, ga[0], ga[1]);
            step3_16(nx, wr, ga[1], ga[0]);
            const int o = rd;
            rd = wr; wr = nx; nx = o;
        }
        if (q < nchunks) step3_16(rd, nx, ga[0], ga[1]);
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = a16[(r >> 2) & 1][2 * j + (r >> 3)][r & 3];
    } else if constexpr (DEPTH == 3) {
        int rd = 0, nx = 1, wr = 2;
        lfrag(0, pk0, f0a, f0b);
        LDS_READS_DONE();
        int q = 0;
        for (; q + 1 < nchunks; q += 2) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                step3(rd, nx);
                const int o = rd;
                rd = nx; nx = wr; wr = o;
            }
        }
        if (q < nchunks) step3(rd, nx);
    } else {
        int q = 0;
        for (; q + 1 < nchunks; q += 2) {
#pragma unroll
            for (int s = 0; s < 2; ++s) step(s);
        }
        if (q < nchunks) step(0);
    }
    // the look-ahead copies of the last chunks still write LDS, and other wavefronts still read their last fragments: the fused
    // GDN, the planes pass and the scale reductions below reuse the ring
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- epilogue: element (j, r) of the lane is local pixel row ROWL(r), local channel COLL(j, r) (MS == 32: column
    // wn0 + 32 j + lr, rows (r & 3) + 8 (r >> 2) + 4 lh of each 32x32 tile; MS == 16: two channels per j, selected by r >> 3) ---
    float *X2 = reinterpret_cast<float *>(smem);                   // [BM][XP]
    float omax = 0.f;                                              // max |output| of this thread
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float bias2[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = COLL(j, h * 8);
            bias2[h] = (a.bias && n < a.N) ? a.bias[n] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = acc[j][r] * fac + bias2[r >> 3];
        if (a.epi == 1) {          // leaky ReLU (slope 0 = ReLU) of a conv + activation pair (layer-wise models)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = acc[j][r] > 0.f ? acc[j][r] : acc[j][r] * a.slope;
        }
    }
    if (a.fuse) {
        // norm[px][i] = beta'[i] + sum_j gamma'[i][j] v[px][j]^2 (gdn.py:52-67): a second contraction, K = N, on the same fp16
        // instruction.  The squares are this workgroup's own data and the contraction runs inside one pixel, so they get a
        // scale of their own from the TILE's maximum (measured, no over-estimate): t = v 2^ev with |t| < 2^7, t^2 < 2^14, split
        // into two fp16 planes and parked in LDS in the A-operand layout of the main loop (one [plane][BM][64 B] image per
        // 32-channel slab); gamma' arrives pre-split as the weight image of a 1x1 convolution (stem_f16x2_pack_conv_weight of the
        // reparametrised matrix, parametrizers.py:42-45; frozen: packed once) and is streamed through one LDS buffer.
        float vm = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) vm = fmaxf(vm, fabsf(acc[j][r]));
        vm = block_max(vm, qred);                          // (its barriers also retire the main loop's last LDS reads)
        const int ev = q_exp(vm) - 8;
        const float vs = q_pow2(ev), vsi = q_pow2(-ev);
        const int nkg = (a.N + KC - 1) / KC;
        unsigned char *Sq = smem;                          // [6][NPL][BM][64 B]
        unsigned char *Bg = smem + 6 * NPL * A_PLANE;      // [NPL][BN][64 B]: one chunk of gamma'
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int slab = (wn0 >> 5) + j;
            if (slab >= nkg) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = ROWL(r), c = COLL(j, r) & 31;                 // channel inside the 32-channel slab
                const float t = acc[j][r] * vs;
                hp_t h0, h1;
                q_split(t * t, 1.f, h0, h1);
                unsigned char *d = Sq + slab * (NPL * A_PLANE) + m * 64 + ((((c >> 3) ^ ((m >> 2) & 3)) << 4) | ((c & 7) << 1));
                *reinterpret_cast<hp_t *>(d) = h0;
                *reinterpret_cast<hp_t *>(d + A_PLANE) = h1;
            }
        }
        f32x16 nrm[3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) nrm[j][r] = 0.f;
        f32x4 n16[2][6];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int nj = 0; nj < 6; ++nj) n16[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
        const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.gp), 0, a.gbytes, 0x00020000);
        f32x4 gb[BP];
        auto gload_g = [&](int kc) {
#pragma unroll
            for (int u = 0; u < BP; ++u) gb[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rg, wv0 + u * (NT * 16), kc * B_BUF, 0));
        };
        gload_g(0);
        for (int kc = 0; kc < nkg; ++kc) {
            __syncthreads();                               // squares written (kc = 0) / previous chunk's fragments read
#pragma unroll
            for (int u = 0; u < BP; ++u) *reinterpret_cast<f32x4 *>(Bg + u * (NT * 16) + tid * 16) = gb[u];
            __syncthreads();
            if (kc + 1 < nkg) gload_g(kc + 1);
            if constexpr (MS == 16) {
                h16x8 A[2][PL], B0[3][PL], B1[3][PL];
                lfragA16(Sq + kc * (NPL * A_PLANE), A);
                lfragB16(Bg, 0, B0);
                lfragB16(Bg, 1, B1);
                mma18(A, B0, 0, n16);
                mma18(A, B1, 1, n16);
                continue;
            }
            const unsigned char *Ab = Sq + kc * (NPL * A_PLANE) + rdA, *Bb = Bg + rdB;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int pk = ks ? pk1 : pk0;
                h16x8 af[NPL], bf[NPL][3];
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) af[pl] = *reinterpret_cast<const h16x8 *>(Ab + pl * A_PLANE + pk);
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
                    for (int j = 0; j < 3; ++j) bf[pl][j] = *reinterpret_cast<const h16x8 *>(Bb + pl * B_PLANE + j * 32 * 64 + pk);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    nrm[j] = STEM_MFMA16(af[1], bf[0][j], nrm[j]);
                    nrm[j] = STEM_MFMA16(af[0], bf[1][j], nrm[j]);
                    nrm[j] = STEM_MFMA16(af[0], bf[0][j], nrm[j]);
                }
            }
        }
        if constexpr (MS == 16) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) nrm[j][r] = n16[(r >> 2) & 1][2 * j + (r >> 3)][r & 3];
        }
        const float gfac = q_inv(a.gq);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float bt2[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = COLL(j, h * 8);
                bt2[h] = 1.f;
                if (n < a.N) {
                    const float bb = fmaxf(a.beta[n], a.beta_bound);
                    bt2[h] = bb * bb - 1.4551915228366852e-11f;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] *= __builtin_amdgcn_rsqf(nrm[j][r] * gfac * vsi * vsi + bt2[r >> 3]);
        }
        __syncthreads();                                   // the parked squares are free (the planes pass reuses the front of LDS)
    }
    if (a.yq) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (COLL(j, r) < a.N && bm0 + ROWL(r) < Mtot) omax = fmaxf(omax, fabsf(acc[j][r]));
        omax = block_max(omax, qred);                      // tail_record (f16x3_tail.h) in place: through the helper the compiler
        if (tid == 0) {                                    // re-orders scalar code inside the fused-GDN section above
            a.yq[QREC_HDR + blockIdx.x] = omax;
            if (blockIdx.x == 0) {
                q_header(a.yq, gridDim.x);
                if (!a.yp) a.yq[1] = 1.f;
            }
        }
    }

    if (a.y) {      // fp32 NHWC output (last layer of the transform)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = bm0 + ROWL(r), n = COLL(j, r);
                if (m < Mtot && n < a.N) a.y[(size_t)m * a.ldy + n] = acc[j][r];
            }
    }
    if (a.yp) {     // planes output for the next convolution: through LDS so that every thread stores whole 16-byte pieces
        __syncthreads();                                   // the parked tile / the main-loop buffers are free
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) X2[ROWL(r) * XP + COLL(j, r)] = acc[j][r];
        __syncthreads();
        const int oslab = a.N / KC, opix = oslab * SLAB;
        unsigned char *yp = static_cast<unsigned char *>(a.yp);
        for (int e = tid; e < BM * oslab * 4; e += NT) {
            const int row = e / (oslab * 4), rem = e - row * (oslab * 4), sl = rem >> 2, p = rem & 3;
            const int m = bm0 + row;
            if (m >= Mtot) continue;
            planes_store8(&X2[row * XP + sl * 32 + p * 8], oscale, yp + (size_t)m * opix + sl * SLAB + p * 16);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// General variant for the small-M layers of the STEM network at training time (16x16 latents: 4096 pixels per batch of 16):
// 64 pixels x 128 channels per workgroup (4 wavefronts as 2 x 2, each 32 x 64), N tiles over blockIdx.y, split-K over
// blockIdx.z with the in-kernel last-arriver reduction of igemm.hip (agent-scope partials, integer ticket, fixed summation
// order), 72 KiB of LDS so that two workgroups share a CU.  Epilogue through an LDS tile: bias, leaky ReLU or its derivative
// (dgrad of a conv whose input was activated), fp32 rows with a pitch (the result may be a channel slice of a wider buffer)
// and / or planes for the next layer.  That tail is stated in f16x3_tail.h (the arrival: splitk_arrive, stem_common.h) and shared
// with conv_f16x3_img_kernel; this file keeps the scatter (ROWL / COLL), the rows' map (OROW) and its own words for the slab sum.
// Weights: the gen image (f16x3_layout.h); the four phases of a transposed face: tconv_axis.
// LDS of a GBM-pixel tile: main loop 2 x (GBM + 128) rows x 64 B x NPL planes, reused by the GBM x 132 float epilogue tile; + tap table
// 16x16x32 by default: alone the STEM layers are 0-8 % slower with it (more issue slots), inside the training step -- a loaded,
// power-limited chip -- the step is 0.2 ms faster
constexpr bool GEN_DEFAULT_MFMA16 = true;
constexpr int glds_main(int gbm) { return 2 * NPL * (gbm + GBN) * 64 > gbm * GTP * 4 ? 2 * NPL * (gbm + GBN) * 64 : gbm * GTP * 4; }
constexpr int glds(int gbm) { return glds_main(gbm) + 32 * 4; }          // 49280 (64 pixels: three workgroups per CU) / 67712 (128: two)

// GBM = pixels per workgroup: 64 (4 wavefronts as 2 x 2) or 128 (8 wavefronts as 4 x 2).  The weight tile of a chunk (16 KB) is
// fetched once per workgroup: with three products per fp32 product the 64-pixel form is bound by that L2 -> LDS traffic
// (24 KB per chunk for 1.6 MF), the 128-pixel form moves 32 KB for twice the work.
// MS = rows of the MFMA shape (see conv_f16x3_kernel): 32, or 16 = v_mfma_f32_16x16x32_f16 with the permuted accumulator layout
// PH: the launch covers the four sub-pixel phases of a transposed face (Fx3Args::ph; host: stem_tconv2d_f16x3_fwd)
template <int GBM, int MS, bool PH = false>
__global__ __launch_bounds__(GBM * 4, 2) void conv_f16x3_gen_kernel(const Fx3Args a)
{
    static_assert(MS == 32 || MS == 16, "MFMA shape");
    int bxt = blockIdx.x, phase = 0;
    if constexpr (PH) {
        phase = blockIdx.x / a.ptiles;
        bxt = blockIdx.x - phase * a.ptiles;
    }
    const int ntaps = PH ? a.ph[phase].ntaps : a.ntaps, tapS = PH ? a.ph[phase].S : a.S;
    const int cps = PH ? a.ph[phase].cps : a.cps, nsplit = PH ? a.ph[phase].nsplit : a.nsplit;
    const int pdy0 = PH ? a.ph[phase].dy0 : (int)a.dy[0], pdx0 = PH ? a.ph[phase].dx0 : (int)a.dx[0];
    const int wofs = PH ? a.ph[phase].wofs : 0;
    if constexpr (PH) {
        if ((int)blockIdx.z >= nsplit) return;        // the whole workgroup: this phase has fewer splits than the launch's z extent
    }
    float *const wsb = PH ? a.ws + a.ph[phase].wsofs : a.ws;
    constexpr int GNT = GBM * 4, GA_PLANE = GBM * 64, GA_BUF = NPL * GA_PLANE;
    constexpr int PL = NPL, BPC = NPL * GBN * 4 / GNT;         // planes; 16-byte weight pieces per thread and chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *As = smem;                        // [2][NPL][GBM][64 B]
    unsigned char *Bs = smem + 2 * GA_BUF;           // [2][NPL][128][64 B]
    int *tapi = reinterpret_cast<int *>(smem + glds_main(GBM));

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Mtot = a.B * a.OH * a.OW;
    const int bm0 = bxt * GBM, bn0 = blockIdx.y * GBN, zsplit = blockIdx.z;
    const int nslab = a.C / KC, pixbytes = a.xpix;

    const int srow = tid >> 2, scol = (tid & 3) ^ ((srow >> 2) & 3);          // LDS row; source piece of this lane's slot (see conv_f16x3_kernel)
    int pb;
    unsigned pmask = 0;
    {
        const int m = bm0 + srow;
        const bool ok = m < Mtot;
        const int mm = ok ? m : 0;
        const int ohw = a.OH * a.OW, b = mm / ohw, rem = mm - b * ohw, qy = rem / a.OW, qx = rem - qy * a.OW;
        const int by = qy * a.stride, bx = qx * a.stride;
        pb = ((b * a.H + by) * a.W + bx) * pixbytes + scol * 16;
        for (int t = 0; t < ntaps; ++t) {
            const int iy = by + (PH ? pdy0 + t / tapS : (int)a.dy[t]), ix = bx + (PH ? pdx0 + t % tapS : (int)a.dx[t]);
            if (ok && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) pmask |= 1u << t;
        }
    }
    const int nchunks = ntaps * nslab;
    const int q_begin = zsplit * cps;
    const int q_end = q_begin + cps < nchunks ? q_begin + cps : nchunks;
    const int q_last = q_end - 1;
    const int wbase = blockIdx.y * nchunks;          // this N tile's chunk sequence inside the packed weights
    __syncthreads();

    const rsrc4 rx = dma_rsrc(a.xp, a.xbytes), rw = dma_rsrc(a.wp, a.wbytes);
    const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char *)smem;
    const unsigned ldsw = __builtin_amdgcn_readfirstlane(lds0 + wave * 1024);
    // chunk q -> LDS stage `stage` by LDS-DMA (see conv_f16x3_kernel): PL + BPC instructions per wavefront
    auto dma = [&](int stage, int t, int tA, int kc, int q) {
        const int sA = kc * SLAB, sB = wofs + (wbase + q) * GB_BUF;
        const int mk = __builtin_amdgcn_sbfe((int)pmask, (unsigned)t, 1u);
        const int off = ((pb + tA) & mk) | (OOR & ~mk);
        const unsigned la = ldsw + stage * GA_BUF, lb = ldsw + 2 * GA_BUF + stage * GB_BUF;
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) dma16(rx, la + pl * GA_PLANE, off + pl * 64, sA);
#pragma unroll
        for (int j = 0; j < BPC; ++j) dma16(rw, lb + j * (GNT * 16), tid * 16 + j * (GNT * 16), sB);
    };

    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 64;
    const int lr = lane & 31, lh = lane >> 5;
    const int sw = (lr >> 2) & 3;
    const int rdA = (wm0 + lr) * 64, rdB = (wn0 + lr) * 64;
    const int pk0 = ((0 + lh) ^ sw) << 4, pk1 = ((2 + lh) ^ sw) << 4;
    // MS == 16: lane l holds channels 16 nj + cm and pixel rows 16 mi + rq + i of the wavefront's 32 x 64 tile
    const int l16 = lane & 15, lq = lane >> 4;
    const int cm = 4 * pi4(l16 >> 2) + (l16 & 3), rq = 4 * pi4(lq);
    const int rdA16 = (wm0 + cm) * 64 + ((lq ^ pi4(l16 >> 2)) << 4), rdB16 = (wn0 + cm) * 64 + ((lq ^ pi4(l16 >> 2)) << 4);
    auto ROWL = [&](int r) { return MS == 32 ? wm0 + (r & 3) + 8 * (r >> 2) + 4 * lh : wm0 + ((r >> 2) & 1) * 16 + rq + (r & 3); };
    auto COLL = [&](int j, int r) { return MS == 32 ? wn0 + j * 32 + lr : wn0 + j * 32 + (r >> 3) * 16 + cm; };
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    int pf_q = 0, pf_t = 0, pf_kc = 0, pf_ts = 0, pf_to = 0;          // see conv_f16x3_kernel
    const int tw_T = ntaps, tw_S = tapS, tw_col = pixbytes, tw_line = a.W * pixbytes, tw_first = (pdy0 * a.W + pdx0) * pixbytes;
    // Two stages: chunk c + 1 is copied into the other stage (free since the barrier that ended chunk c - 1) while chunk c is
    // multiplied, and has landed for every wavefront behind the wait and the barrier that end the step; the other workgroups of
    // the CU cover what the one chunk of look-ahead does not
    auto step = [&](int cur) {
        const unsigned char *Ab = As + cur * GA_BUF + rdA, *Bb = Bs + cur * GB_BUF + rdB;
        const int t = __builtin_amdgcn_readfirstlane(pf_t), kc = __builtin_amdgcn_readfirstlane(pf_kc), q = __builtin_amdgcn_readfirstlane(pf_q);
        const int to = __builtin_amdgcn_readfirstlane(pf_to);
        dma(cur ^ 1, t, to, kc, q);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pk = ks ? pk1 : pk0;
            h16x8 af[PL], bf[PL][2];
#pragma unroll
            for (int pl = 0; pl < PL; ++pl) af[pl] = *reinterpret_cast<const h16x8 *>(Ab + pl * GA_PLANE + pk);
#pragma unroll
            for (int pl = 0; pl < PL; ++pl)
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[pl][j] = *reinterpret_cast<const h16x8 *>(Bb + pl * GB_PLANE + j * 32 * 64 + pk);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[j] = STEM_MFMA16(af[1], bf[0][j], acc[j]);
                acc[j] = STEM_MFMA16(af[0], bf[1][j], acc[j]);
                acc[j] = STEM_MFMA16(af[0], bf[0][j], acc[j]);
            }
        }
        if (pf_q < q_last) TAP_WALK_NEXT();
        DMA_WAIT_BARRIER(0);
    };
    // MS == 16: a chunk is one k-step of the 16x16x32 instruction; 2 x 4 accumulators of four registers, the eight independent
    // accumulators of a product back to back
    f32x4 a16[2][4];
    if constexpr (MS == 16) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) a16[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    auto step16 = [&](int cur) {
        const unsigned char *Ab = As + cur * GA_BUF + rdA16, *Bb = Bs + cur * GB_BUF + rdB16;
        const int t = __builtin_amdgcn_readfirstlane(pf_t), kc = __builtin_amdgcn_readfirstlane(pf_kc), q = __builtin_amdgcn_readfirstlane(pf_q);
        const int to = __builtin_amdgcn_readfirstlane(pf_to);
        dma(cur ^ 1, t, to, kc, q);
        h16x8 A[2][PL], B[4][PL];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int pl = 0; pl < PL; ++pl) A[mi][pl] = *reinterpret_cast<const h16x8 *>(Ab + mi * 16 * 64 + pl * GA_PLANE);
#pragma unroll
        for (int nj = 0; nj < 4; ++nj)
#pragma unroll
            for (int pl = 0; pl < PL; ++pl) B[nj][pl] = *reinterpret_cast<const h16x8 *>(Bb + nj * 16 * 64 + pl * GB_PLANE);
#pragma unroll
        for (int prod = 0; prod < 3; ++prod)            // smallest terms first
#pragma unroll
            for (int nj = 0; nj < 4; ++nj)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    a16[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[mi][prod == 0 ? 1 : 0], B[nj][prod == 1 ? 1 : 0], a16[mi][nj], 0, 0, 0);
        if (pf_q < q_last) TAP_WALK_NEXT();
        DMA_WAIT_BARRIER(0);
    };
    // A wavefront whose 64 columns lie entirely beyond N (the second column pair of the last tile of a 320-channel layer: a
    // sixth of the launch's matrix work) only takes part in the staging: same copies and barriers, no LDS reads and
    // no MFMAs.  The choice is made once per wavefront, OUTSIDE the woven block (a per-sub-tile branch inside it was slower).
    const bool dead = bn0 + wn0 >= a.N;
    auto step_dead = [&](int cur) {
        const int t = __builtin_amdgcn_readfirstlane(pf_t), kc = __builtin_amdgcn_readfirstlane(pf_kc), q = __builtin_amdgcn_readfirstlane(pf_q);
        const int to = __builtin_amdgcn_readfirstlane(pf_to);
        dma(cur ^ 1, t, to, kc, q);
        if (pf_q < q_last) TAP_WALK_NEXT();
        DMA_WAIT_BARRIER(0);
    };
    auto chunk_of = [&](int q, int &t, int &kc) {
        q = q < q_last ? q : q_last;
        kc = q / ntaps;
        t = q - kc * ntaps;
        return q;
    };
    if (q_begin < q_end) {
        int t, kc, q;
        q = chunk_of(q_begin, t, kc);
        dma(0, t, TAP_OFFSET(t), kc, q);
        pf_q = chunk_of(q_begin + 1, pf_t, pf_kc);
        pf_ts = pf_t % tw_S;
        pf_to = TAP_OFFSET(pf_t);
    }
    // scales of the epilogue, computed while the first chunks are in flight (see conv_f16x3_kernel; every split of a tile
    // computes the same values, the last arriver uses them)
    __shared__ float qred[16];
    const float fac = q_inv(a.xq) * q_inv(a.wq);                   // the operands were stored times 2^ex, 2^ew
    const float oscale = tail_oscale<GNT>(a.yp != nullptr, a.xq, a.wq, a.bias, a.N, a.C * (PH ? a.btaps : ntaps), a.yq, blockIdx.x == 0 && blockIdx.y == 0, qred);
    __syncthreads();
    DMA_WAIT_BARRIER(0);            // the first chunk has landed, for every wavefront
    if (!dead && MS == 16) {
        int q = q_begin;
        for (; q + 1 < q_end; q += 2) {
            step16(0);
            step16(1);
        }
        if (q < q_end) step16(0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = a16[(r >> 2) & 1][2 * j + (r >> 3)][r & 3];
    } else if (!dead) {
        int q = q_begin;
        for (; q + 1 < q_end; q += 2) {
            step(0);
            step(1);
        }
        if (q < q_end) step(0);
    } else {
        int q = q_begin;
        for (; q + 1 < q_end; q += 2) {
            step_dead(0);
            step_dead(1);
        }
        if (q < q_end) step_dead(0);
    }
    // every step ends with its copy landed and a barrier: nothing is in flight, and nobody still reads the ring the tail reuses

    // ---- the tail (f16x3_tail.h).  Stated here: the scatter of the accumulators, tile row -> output row (OROW), the slab sum ----
    float *T = reinterpret_cast<float *>(smem);                     // [GBM][GTP]
    const int Npad = gridDim.y * GBN;
    constexpr int ERS = GNT / 32, ER = GBM / ERS;                   // 8 pieces per thread
    const int ec4 = tid & 31, er0 = tid >> 5;
    f32x4 ev[ER];
    // output pixel of tile row `row` or -1: m itself, or -- phases -- fine pixel (2 qy + py, 2 qx + px) inside the (odd) OHf x OWf
    auto OROW = [&](int row) -> long {
        const int m = bm0 + row;
        if (m >= Mtot) return -1;
        if constexpr (!PH) return m;
        const int ohw = a.OH * a.OW, b = m / ohw, rem = m - b * ohw, qy = rem / a.OW, qx = rem - qy * a.OW;
        const int oy = 2 * qy + a.ph[phase].ooy, ox = 2 * qx + a.ph[phase].oox;
        return oy < a.OHf && ox < a.OWf ? ((long)b * a.OHf + oy) * a.OWf + ox : -1;
    };
    if (nsplit > 1) {
        float *wsp = wsb + (size_t)zsplit * Mtot * Npad;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = bm0 + ROWL(r), n = bn0 + COLL(j, r);
                if (m < Mtot) __hip_atomic_store(&wsp[(size_t)m * Npad + n], acc[j][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (!splitk_arrive(a.cnt + blockIdx.y * gridDim.x + blockIdx.x, nsplit, tapi)) return;
        constexpr int SC1 = 16;               // sc1: read at the device-coherent level, not this XCD's L2
        const __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc(wsb, 0, (int)((size_t)nsplit * Mtot * Npad * 4), 0x00020000);
        const int sstep = Mtot * Npad * 4;
        // tail_slab_sum<ER, 4> in this kernel's own words: 4 pieces x 4 splits in flight.  Through the helper, in every form of it
        // that was tried, conv_f16x3_gen_kernel<128, 32> takes 114 vector registers instead of 112.
        int eoff[ER];
#pragma unroll
        for (int k = 0; k < ER; ++k) {
            const int m = bm0 + er0 + ERS * k;
            eoff[k] = m < Mtot ? (m * Npad + bn0 + ec4 * 4) * 4 : OOR;
        }
#pragma unroll
        for (int k = 0; k < ER; ++k) ev[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < ER; kb += 4)
            for (int sp = 0; sp < nsplit; sp += 4) {
                f32x4 tt[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        tt[k][u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rws, sp + u < nsplit ? eoff[kb + k] : OOR,
                                                                                                      (sp + u < nsplit ? sp + u : 0) * sstep, SC1));
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int u = 0; u < 4; ++u) ev[kb + k] += tt[k][u];          // beyond nsplit: zeros (out-of-range loads)
            }
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) T[ROWL(r) * GTP + COLL(j, r)] = acc[j][r];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ER; ++k) ev[k] = *reinterpret_cast<const f32x4 *>(&T[(er0 + ERS * k) * GTP + ec4 * 4]);
    }
    const int ecol = bn0 + (tid & 31) * 4;
    float omax = tail_rows<GBM, GNT>(a, ev, T, ecol, fac, tail_bias4(a.bias, ecol, a.N), OROW);
    tail_record(a.yq, a.yp != nullptr, omax, qred, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
    if (a.yp) {
        __syncthreads();
        const int oslab = a.N / KC, opix = oslab * SLAB;
        unsigned char *yp = static_cast<unsigned char *>(a.yp);
        for (int e = tid; e < GBM * (GBN / 8); e += GNT) {
            const int row = e / (GBN / 8), c8 = e - row * (GBN / 8), n = bn0 + c8 * 8;
            const long m = OROW(row);
            if (m < 0 || n >= a.N) continue;                // N % 32 == 0 for planes (host check)
            planes_store8(&T[row * GTP + c8 * 8], oscale, yp + m * opix + (n >> 5) * SLAB + ((n >> 3) & 3) * 16);
        }
    }
}

}   // namespace

static int conv2d_f16x3_launch(const void *xp, const float *xq, const void *wp, const float *bias, const float *beta, const void *gp,
                                float beta_min, int act, float slope, float *y, int ldy, void *yp, float *yq, int B, int H, int W, int C, int N,
                                int R, int S, int stride, int pad, void *stream);

STEM_EXPORT int stem_conv2d_f16x3_fwd(const void *xp, const float *xq, const void *wp, const float *bias, const float *beta, const void *gp,
                                       float beta_min, float *y, int ldy, void *yp, float *yq, int B, int H, int W, int C, int N, int R, int S,
                                       int stride, int pad, void *stream)
{
    return conv2d_f16x3_launch(xp, xq, wp, bias, beta, gp, beta_min, 0, 0.f, y, ldy, yp, yq, B, H, W, C, N, R, S, stride, pad, stream);
}

STEM_EXPORT int stem_conv2d_f16x3_fwd_act(const void *xp, const float *xq, const void *wp, const float *bias, int act, float slope, float *y, int ldy,
                                           void *yp, float *yq, int B, int H, int W, int C, int N, int R, int S, int stride, int pad, void *stream)
{
    STEM_CHECK_ARG(act == 0 || act == 1, "stem_conv2d_f16x3_fwd_act: act is 0 (none) or 1 (leaky ReLU with `slope`)");
    STEM_CHECK_ARG(!act || fabsf(slope) <= 1.f, "stem_conv2d_f16x3_fwd_act: |slope| <= 1");
    return conv2d_f16x3_launch(xp, xq, wp, bias, nullptr, nullptr, 1e-6f, act, slope, y, ldy, yp, yq, B, H, W, C, N, R, S, stride, pad, stream);
}

static int conv2d_f16x3_launch(const void *xp, const float *xq, const void *wp, const float *bias, const float *beta, const void *gp,
                                float beta_min, int act, float slope, float *y, int ldy, void *yp, float *yq, int B, int H, int W, int C, int N,
                                int R, int S, int stride, int pad, void *stream)
{
    STEM_CHECK_ARG(xp && xq && wp && (y || yp) && (yq || !yp), "stem_conv2d_f16x3_fwd: null pointer (planes come with their scale records)");
    STEM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 32 && C % 32 == 0 && N >= 1 && N <= BN && R >= 1 && S >= 1 && R * S <= MAXTAP &&
                   stride >= 1 && pad >= 0, "stem_conv2d_f16x3_fwd: C %% 32 == 0, N <= %d, R*S <= %d (C=%d N=%d R=%d S=%d)", BN, MAXTAP, C, N, R, S);
    STEM_CHECK_ARG(!yp || N % 32 == 0, "stem_conv2d_f16x3_fwd: planes output needs N %% 32 == 0 (N=%d)", N);
    STEM_CHECK_ARG(!y || ldy >= N, "stem_conv2d_f16x3_fwd: ldy < N");
    STEM_CHECK_ARG((beta == nullptr) == (gp == nullptr), "stem_conv2d_f16x3_fwd: beta and the packed gamma come together");
    const int OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
    STEM_CHECK_ARG(OH >= 1 && OW >= 1, "stem_conv2d_f16x3_fwd: empty output");
    const size_t xb = planes_payload((long)B * H * W, C), wb = w_image_bytes(C, R, S);
    STEM_CHECK_ARG(xb < 0x7FFFFF00ull && wb < 0x7FFFFF00ull && (size_t)B * OH * OW < 0x7FFFFFFFull,
                   "stem_conv2d_f16x3_fwd: operand views must stay below 2 GiB (split the batch)");
    Fx3Args a;
    memset(&a, 0, sizeof(a));
    a.xp = xp; a.wp = wp; a.bias = bias; a.beta = beta; a.gp = gp; a.y = y; a.yp = yp; a.ldy = ldy;
    if (gp) {       // gamma' = the packed image of an [N][ceil32(N)] 1x1 weight, its scale record behind it
        const int cpad = cdiv(N, 32) * 32;
        a.gbytes = (int)w_image_bytes(cpad, 1, 1);
        a.gq = reinterpret_cast<const float *>(static_cast<const unsigned char *>(gp) + a.gbytes);
    }
    a.xq = xq; a.yq = yq; a.wq = reinterpret_cast<const float *>(static_cast<const unsigned char *>(wp) + wb);
    a.B = B; a.H = H; a.W = W; a.C = C; a.N = N; a.OH = OH; a.OW = OW; a.stride = stride; a.ntaps = R * S; a.S = S;
    a.xbytes = (int)xb; a.wbytes = (int)wb;
    a.fuse = gp ? 1 : 0;
    a.epi = act; a.slope = slope;
    a.beta_bound = (float)sqrt((double)beta_min + 1.4551915228366852e-11);
    for (int r = 0; r < R; ++r)
        for (int s = 0; s < S; ++s) {
            a.dy[r * S + s] = (signed char)(r - pad);
            a.dx[r * S + s] = (signed char)(s - pad);
        }
    static bool attr_done = false;      // > 64 KiB of dynamic LDS needs an explicit opt-in
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)conv_f16x3_kernel<128, 2, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_total(128, 2));
        (void)hipFuncSetAttribute((const void *)conv_f16x3_kernel<128, 3, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_total(128, 3));
        (void)hipFuncSetAttribute((const void *)conv_f16x3_kernel<128, 3, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_total(128, 3));
        (void)hipFuncSetAttribute((const void *)conv_f16x3_kernel<64, 2, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_total(64, 2));
        (void)hipFuncSetAttribute((const void *)conv_f16x3_kernel<64, 3, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_total(64, 3));
        (void)hipFuncSetAttribute((const void *)conv_f16x3_kernel<64, 3, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_total(64, 3));
        attr_done = true;
    }
    const int M = B * OH * OW;
    hipStream_t st = (hipStream_t)stream;
    // 128-pixel tiles (8 wavefronts) when there is one for at least half of the 256 CUs, 64-pixel tiles (4 wavefronts) below
    // that.  Alone, 64-pixel tiles are faster up to 255 tiles (g_a.4 at B=16, 128 tiles: 127 against 140 us); next to other
    // streams' work -- where such a launch runs in the training step -- one workgroup per CU on half the chip beats two small
    // ones per CU everywhere (bench step 15.46-15.54 -> 15.27-15.33 ms), so the threshold follows the loaded machine.
    const int tile = stem_tuning(STEM_TUNE_FX3_TILE);
    const bool small = tile ? tile == 64 : cdiv(M, 128) < 128;
    // main-loop form (see the kernel): stem_tuning_set("fx3_depth", 2 | 3); 0 = default
    // default: three stages with 128-pixel tiles (g_a.2 365 -> 357 us), two with 64-pixel tiles -- 96 KB of LDS would leave room
    // for ONE such workgroup per CU, and layers with 256 .. 511 tiles (g_a.4) run two per CU next to other streams' work
    const int dsel = stem_tuning(STEM_TUNE_FX3_DEPTH);
    const int depth = dsel ? dsel : (small ? 2 : 3);
    // MFMA shape (see the kernel): 16x16x32 where the launch fills the chip with 128-pixel tiles and runs the three-stage loop,
    // 32x32x16 otherwise; stem_tuning_set("fx3_mfma", 16 | 32) forces it where the loop form allows
    const int msel = stem_tuning(STEM_TUNE_FX3_MFMA);
    const bool m16 = depth == 3 && (msel ? msel == 16 : !small);
    stem_ran_note(STEM_RAN_FX3_COL_TILE, small ? 64 : 128);      // test aids: stem_tuning_get("fx3_col_ran_tile" | "fx3_col_ran_depth" | "fx3_col_ran_mfma")
    stem_ran_note(STEM_RAN_FX3_COL_DEPTH, depth == 3 ? 3 : 2);
    stem_ran_note(STEM_RAN_FX3_COL_MFMA, m16 ? 16 : 32);
    if (small && m16)
        hipLaunchKernelGGL((conv_f16x3_kernel<64, 3, 16>), dim3(cdiv(M, 64)), dim3(256), lds_total(64, 3), st, a);
    else if (small && depth == 3)
        hipLaunchKernelGGL((conv_f16x3_kernel<64, 3, 32>), dim3(cdiv(M, 64)), dim3(256), lds_total(64, 3), st, a);
    else if (small)
        hipLaunchKernelGGL((conv_f16x3_kernel<64, 2, 32>), dim3(cdiv(M, 64)), dim3(256), lds_total(64, 2), st, a);
    else if (m16)
        hipLaunchKernelGGL((conv_f16x3_kernel<128, 3, 16>), dim3(cdiv(M, 128)), dim3(512), lds_total(128, 3), st, a);
    else if (depth == 3)
        hipLaunchKernelGGL((conv_f16x3_kernel<128, 3, 32>), dim3(cdiv(M, 128)), dim3(512), lds_total(128, 3), st, a);
    else
        hipLaunchKernelGGL((conv_f16x3_kernel<128, 2, 32>), dim3(cdiv(M, 128)), dim3(512), lds_total(128, 2), st, a);
    STEM_LAUNCH_CHECK("stem_conv2d_f16x3_fwd");
    return 0;
}

// ---- general variant: N tiles of 128, split-K, activation epilogues (training-time STEM layers) --------------------------------
namespace {
constexpr size_t kGenCntBytes = 64 * 1024;          // arrival counters in front of the split-K slabs: the layout of igemm.hip's
                                                    // workspace, so that one zero-headed buffer per stream serves both kernels

// Split factor.  Two workgroups fit a CU; the launch runs in R = ceil(workgroups / 256) "CU rounds", each as long as one
// workgroup's chunks (+ ~6 chunks of ramp-up per workgroup) -- except that a lone workgroup per CU (R = 1) leaves the matrix
// pipes ~40 % idle (one wavefront per SIMD).  Every split also pays its slab in the reduction.  Measured on TPM.0 / .2 / .4
// with splits 1..10 (tools/debug/f16x3_gen_check.py, STEM_FX3_SPLIT): the model ranks them as measured, optimum 4 / 4 / 4.
int gen_split(int tiles, int nchunks)
{
    const int forced = stem_tuning(STEM_TUNE_FX3_SPLIT);      // stem_tuning_set("fx3_split", n): tests / sweeps
    if (forced > 0) return forced < nchunks ? forced : nchunks;
    // 1x1 layers (EPM: 18-36 chunks): a split costs its slab round trip and a second epilogue pass, more than the shorter loop
    // returns (tools/debug/f16x3_split_sweep.py, round 3: unsplit 39 / 29 / 20 us against 43 / 33 / 26 us)
    if (nchunks <= 40 && tiles >= 128) return 1;
    int best = 1;
    double best_cost = 1e30;
    for (int s = 1; s <= 16 && s * 8 <= nchunks; ++s) {
        const int cps = cdiv(nchunks, s), ns = cdiv(nchunks, cps), rounds = cdiv(tiles * ns, 256);
        const double cost = rounds * (cps + 6.0) * (rounds == 1 ? 1.67 : 1.0) + (ns > 1 ? 0.3 * ns : 0.0);
        if (cost < best_cost - 1e-9) {
            best_cost = cost;
            best = ns;
        }
    }
    return best;
}

// Pixel tile: 128 when that still leaves enough tiles to spread over the chip with a moderate split and the loop is long enough
// to pay for the larger epilogue, else 64 (tools/debug/f16x3_split_sweep.py: TPM.0 / .2 / .4 52 / 78 / 100 -> 49 / 73 / 90 us,
// EPM.0 / .2 41 / 31 -> 38 / 28 us, EPM.4 with its 18 chunks 20 -> 23 us)
int gen_bm(int M, int ntn, int nchunks)
{
    const int forced = stem_tuning(STEM_TUNE_FX3_GEN_TILE);   // stem_tuning_set("fx3_gen_tile", 64 | 128): tests / sweeps
    if (forced) return forced;
    // (the nchunks > 20 clause of the isolated sweep is gone: inside the training step the short 1x1 launches -- EPM.2 / EPM.4 and
    // the EPM input gradients, 22-26 us on either tile alone -- run 0.07 ms per step faster on the larger workgroups, six
    // alternating pairs 15.21-15.26 against 15.16-15.20 ms: fewer, larger workgroups share the loaded chip better)
    (void)nchunks;
    return cdiv(M, 128) * ntn >= 64 ? 128 : 64;
}
}   // namespace

STEM_EXPORT size_t stem_conv2d_f16x3_gen_workspace_bytes(int B, int H, int W, int C, int N, int R, int S, int stride, int pad, int taps)
{
    const int OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
    if (OH < 1 || OW < 1 || C % 32) return 0;
    const int M = B * OH * OW, nchunks = (C / 32) * (taps > 0 ? taps : R * S), tiles = cdiv(M, gen_bm(M, cdiv(N, GBN), nchunks)) * cdiv(N, GBN);
    int s = gen_split(tiles, nchunks);
    if (stem_fx3_img_eligible(B, H, W, N, R, S, stride, pad)) {       // the image-tile form plans its own split: room for either
        const int si = stem_fx3_img_split(stem_fx3_img_tiles(B, H, W, N), nchunks);
        if (si > s) s = si;
    }
    while (s > 1 && (size_t)s * M * cdiv(N, GBN) * GBN * sizeof(float) >= 0x7FFFFF00ull) --s;
    return s > 1 ? kGenCntBytes + (size_t)s * M * cdiv(N, GBN) * GBN * sizeof(float) : 0;
}

STEM_EXPORT int stem_conv2d_f16x3_gen_fwd(const void *xp, const float *xq, int xpix, const void *wp, const float *bias, int epi, float slope,
                                           const float *z, int ldz, float *y, int ldy, void *yp, float *yq, int B, int H, int W, int C, int N, int R,
                                           int S, int stride, int pad, int taps, void *ws, size_t ws_bytes, void *stream)
{
    STEM_CHECK_ARG(taps >= 0 && taps <= R * S, "stem_conv2d_f16x3_gen_fwd: 0 <= taps <= R*S (taps=%d)", taps);
    const int T = taps > 0 ? taps : R * S;
    STEM_CHECK_ARG(xp && xq && wp && (y || yp) && (yq || !yp), "stem_conv2d_f16x3_gen_fwd: null pointer (planes come with their scale records)");
    STEM_CHECK_ARG(epi == GEN_EPI_BIAS || fabsf(slope) <= 1.f, "stem_conv2d_f16x3_gen_fwd: |slope| <= 1");
    STEM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 32 && C % 32 == 0 && N >= 4 && N % 4 == 0 && R >= 1 && S >= 1 && R * S <= MAXTAP &&
                   stride >= 1 && pad >= 0, "stem_conv2d_f16x3_gen_fwd: C %% 32 == 0, N %% 4 == 0, R*S <= %d (C=%d N=%d R=%d S=%d)", MAXTAP, C, N, R, S);
    STEM_CHECK_ARG(!yp || N % 32 == 0, "stem_conv2d_f16x3_gen_fwd: planes output needs N %% 32 == 0 (N=%d)", N);
    STEM_CHECK_ARG(!y || (ldy >= N && ldy % 4 == 0 && ((uintptr_t)y & 15) == 0), "stem_conv2d_f16x3_gen_fwd: y rows must be 16-byte aligned, ldy >= N");
    STEM_CHECK_ARG(epi >= GEN_EPI_BIAS && epi <= GEN_EPI_DACT, "stem_conv2d_f16x3_gen_fwd: unknown epilogue %d", epi);
    STEM_CHECK_ARG(epi != GEN_EPI_DACT || (z && ldz >= N && ldz % 4 == 0 && ((uintptr_t)z & 15) == 0), "stem_conv2d_f16x3_gen_fwd: DACT needs z (16-byte aligned rows)");
    const int OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
    STEM_CHECK_ARG(OH >= 1 && OW >= 1, "stem_conv2d_f16x3_gen_fwd: empty output");
    if (xpix == 0) xpix = (C / 32) * SLAB;
    STEM_CHECK_ARG(xpix >= (C / 32) * SLAB && xpix % SLAB == 0, "stem_conv2d_f16x3_gen_fwd: xpix must be a multiple of %d bytes covering C channels", SLAB);
    const size_t xb = (size_t)B * H * W * xpix, wb = gen_image_bytes(N, C, R, S);
    const int M = B * OH * OW, ntn = cdiv(N, GBN), nchunks = (C / 32) * T, bm = gen_bm(M, ntn, nchunks), tiles = cdiv(M, bm) * ntn;
    STEM_CHECK_ARG(xb < 0x7FFFFF00ull && wb < 0x7FFFFF00ull && (size_t)M * ntn * GBN * 4 < 0x7FFFFF00ull,
                   "stem_conv2d_f16x3_gen_fwd: operand views must stay below 2 GiB (split the batch)");
    Fx3Args a;
    memset(&a, 0, sizeof(a));
    a.xp = xp; a.wp = wp; a.bias = bias; a.y = y; a.yp = yp; a.ldy = ldy; a.z = z; a.ldz = ldz; a.epi = epi; a.slope = slope;
    const float *wq = reinterpret_cast<const float *>(static_cast<const unsigned char *>(wp) + wb);
    a.xq = xq; a.yq = yq; a.wq = wq;
    a.B = B; a.H = H; a.W = W; a.C = C; a.N = N; a.OH = OH; a.OW = OW; a.stride = stride; a.ntaps = T; a.S = S;
    a.xbytes = (int)xb; a.wbytes = (int)wb; a.xpix = xpix;
    for (int r = 0; r < R; ++r)
        for (int s = 0; s < S; ++s) {
            a.dy[r * S + s] = (signed char)(r - pad);
            a.dx[r * S + s] = (signed char)(s - pad);
        }
    // stride-1 "same" layers on images of 16x16 blocks: the image-tile form (conv_f16x3_img.hip: halo in LDS, weights by LDS-DMA)
    const bool img = stem_fx3_img_eligible(B, H, W, N, R, S, stride, pad);
    const int itiles = img ? stem_fx3_img_tiles(B, H, W, N) : 0;
    int split = img ? stem_fx3_img_split(itiles, nchunks) : gen_split(tiles, nchunks);
    while (split > 1 && (size_t)split * M * ntn * GBN * sizeof(float) >= 0x7FFFFF00ull) --split;      // the slabs are read through one buffer view
    const size_t need = kGenCntBytes + (size_t)split * M * ntn * GBN * sizeof(float);
    if (split > 1 && (!ws || ws_bytes < need || (size_t)tiles * sizeof(int) > kGenCntBytes)) split = 1;      // no workspace: unsplit, same result up to summation order
    const int cps = cdiv(nchunks, split), nsplit = cdiv(nchunks, cps);
    const int gmsel = stem_tuning(STEM_TUNE_FX3_GEN_MFMA);         // MFMA shape: stem_tuning_set("fx3_gen_mfma", 16 | 32); 0 = default
    const bool g16 = gmsel ? gmsel == 16 : GEN_DEFAULT_MFMA16;
    stem_ran_note(STEM_RAN_FX3_FORM, img ? 3 : bm == 128 ? 2 : 1);      // test aids: stem_tuning_get("fx3_ran_form" | "fx3_ran_split" | "fx3_ran_mfma")
    stem_ran_note(STEM_RAN_FX3_SPLIT, nsplit);
    stem_ran_note(STEM_RAN_FX3_MFMA, !img && g16 ? 16 : 32);
    if (img)
        return stem_fx3_img_launch(xp, xq, xpix, (int)xb, wp, wq, (int)wb,
                                   bias, epi, slope, z, ldz, y, ldy, yp, yq, B, H, W, C, N, R, T, split,
                                   split > 1 ? reinterpret_cast<float *>(static_cast<unsigned char *>(ws) + kGenCntBytes) : nullptr,
                                   split > 1 ? static_cast<int *>(ws) : nullptr, stream);
    a.cps = cps;
    a.nsplit = nsplit;
    if (a.nsplit > 1) {
        a.cnt = static_cast<int *>(ws);
        a.ws = reinterpret_cast<float *>(static_cast<unsigned char *>(ws) + kGenCntBytes);
    }
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)conv_f16x3_gen_kernel<64, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, glds(64));
        (void)hipFuncSetAttribute((const void *)conv_f16x3_gen_kernel<128, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, glds(128));
        (void)hipFuncSetAttribute((const void *)conv_f16x3_gen_kernel<64, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, glds(64));
        (void)hipFuncSetAttribute((const void *)conv_f16x3_gen_kernel<128, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, glds(128));
        attr_done = true;
    }
    const dim3 grid(cdiv(M, bm), ntn, a.nsplit);
    if (bm == 128 && g16)
        hipLaunchKernelGGL((conv_f16x3_gen_kernel<128, 16>), grid, dim3(512), glds(128), (hipStream_t)stream, a);
    else if (bm == 128)
        hipLaunchKernelGGL((conv_f16x3_gen_kernel<128, 32>), grid, dim3(512), glds(128), (hipStream_t)stream, a);
    else if (g16)
        hipLaunchKernelGGL((conv_f16x3_gen_kernel<64, 16>), grid, dim3(256), glds(64), (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((conv_f16x3_gen_kernel<64, 32>), grid, dim3(256), glds(64), (hipStream_t)stream, a);
    STEM_LAUNCH_CHECK("stem_conv2d_f16x3_gen_fwd");
    return 0;
}

namespace {
// chunks per workgroup of a four-phase launch: every workgroup gets (about) the same number of chunks whatever its phase; the
// cost model of gen_split with the phases' workgroups added up
int tconv_cps(int tiles_per_phase, const int (&nchunks)[4])
{
    const int forced = stem_tuning(STEM_TUNE_FX3_SPLIT);
    int maxc = 0;
    for (int p = 0; p < 4; ++p) maxc = nchunks[p] > maxc ? nchunks[p] : maxc;
    if (forced > 0) return cdiv(maxc, forced < maxc ? forced : maxc);
    if (stem_tuning(STEM_TUNE_TCONV_CPS) > 0) return stem_tuning(STEM_TUNE_TCONV_CPS);       // stem_tuning_set("tconv_cps", n): sweeps
    // These launches are latency-bound (tools/debug/tconv_sweep.py, round 5: HD.0 24-29 us and HD.2 38-40 us for 12-24 chunks per
    // workgroup, 49-64 us at 4-8, 45-62 us at 36-72): the shortest loop that keeps the launch within one round of 512 workgroups
    // (two per CU) and the reduction within 16 slabs, but not below 12 chunks -- under that the slab round trip outweighs the loop
    for (int cps = 12; cps < maxc; ++cps) {
        int wgs = 0, maxns = 0;
        for (int p = 0; p < 4; ++p) {
            const int ns = cdiv(nchunks[p], cps);
            wgs += tiles_per_phase * ns;
            maxns = ns > maxns ? ns : maxns;
        }
        if (wgs <= 512 && maxns <= 16) return cps;
    }
    return maxc;
}
}   // namespace

STEM_EXPORT size_t stem_tconv2d_f16x3_workspace_bytes(int B, int H, int W, int C, int N, int R)
{
    if (C % 32 || R < 1 || R * R > MAXTAP || !(R & 1)) return 0;
    const int M = B * H * W, ntn = cdiv(N, GBN);
    // room for any plan: 16 splits of every phase
    return kGenCntBytes + (size_t)4 * 16 * M * ntn * GBN * sizeof(float);
}

/* The transposed face of a stride-2, R x R, padding R/2 layer whose fine grid is exactly twice the coarse one:
 *   forward of nn.ConvTranspose2d(C, N, R, stride=2, padding=R/2, output_padding=1)   (HD.0 / HD.2, spatiotemporalpriors.py:822-826)
 *   input gradient of nn.Conv2d(N, C, R, stride=2, padding=R/2) on an even-sized input   (HE.2 / HE.4, :814-818, torch autograd)
 * x: planes of the coarse tensor [B, H, W, C]; wp: the four phase images (stem_f16x2_pack_conv_weights_multi, flip = 2, rows =
 * the N outputs, contraction channels C); y / yp: fp32 rows / planes of the fine tensor [B, OHf, OWf, N], OHf = 2H (or 2H - 1: the
 * input gradient of a strided convolution whose input had an odd number of rows; same for OWf); epi / z as in
 * stem_conv2d_f16x3_gen_fwd (z: rows of the FINE tensor).  One launch: blockIdx.x = phase x coarse pixel tile. */
STEM_EXPORT int stem_tconv2d_f16x3_fwd(const void *xp, const float *xq, int xpix, const void *wp, const float *bias, int epi, float slope,
                                        const float *z, int ldz, float *y, int ldy, void *yp, float *yq, int B, int H, int W, int C, int N, int R,
                                        int OHf, int OWf, void *ws, size_t ws_bytes, void *stream)
{
    STEM_CHECK_ARG(xp && xq && wp && (y || yp) && (yq || !yp), "stem_tconv2d_f16x3_fwd: null pointer (planes come with their scale records)");
    STEM_CHECK_ARG((OHf == 2 * H || OHf == 2 * H - 1) && (OWf == 2 * W || OWf == 2 * W - 1),
                   "stem_tconv2d_f16x3_fwd: the fine grid is 2H or 2H - 1 rows (the odd-sized input of a strided convolution), got %d x %d for %d x %d", OHf, OWf, H, W);
    STEM_CHECK_ARG(epi >= GEN_EPI_BIAS && epi <= GEN_EPI_DACT && (epi == GEN_EPI_BIAS || fabsf(slope) <= 1.f), "stem_tconv2d_f16x3_fwd: epilogue %d", epi);
    STEM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 32 && C % 32 == 0 && N >= 4 && N % 4 == 0 && R >= 3 && (R & 1) && R * R <= MAXTAP,
                   "stem_tconv2d_f16x3_fwd: C %% 32 == 0, N %% 4 == 0, odd 3 <= R, R*R <= %d (C=%d N=%d R=%d)", MAXTAP, C, N, R);
    STEM_CHECK_ARG(!yp || N % 32 == 0, "stem_tconv2d_f16x3_fwd: planes output needs N %% 32 == 0 (N=%d)", N);
    STEM_CHECK_ARG(!y || (ldy >= N && ldy % 4 == 0 && ((uintptr_t)y & 15) == 0), "stem_tconv2d_f16x3_fwd: y rows must be 16-byte aligned, ldy >= N");
    STEM_CHECK_ARG(epi != GEN_EPI_DACT || (z && ldz >= N && ldz % 4 == 0 && ((uintptr_t)z & 15) == 0), "stem_tconv2d_f16x3_fwd: DACT needs z (16-byte aligned rows)");
    if (xpix == 0) xpix = (C / 32) * SLAB;
    STEM_CHECK_ARG(xpix >= (C / 32) * SLAB && xpix % SLAB == 0, "stem_tconv2d_f16x3_fwd: xpix must be a multiple of %d bytes covering C channels", SLAB);
    const int pad = R / 2, nslab = C / 32, M = B * H * W, ntn = cdiv(N, GBN);
    const size_t xb = (size_t)B * H * W * xpix, wb = gen_image_bytes(N, C, R, R);
    STEM_CHECK_ARG(xb < 0x7FFFFF00ull && wb < 0x7FFFFF00ull && (size_t)4 * M * ntn * GBN * 4 < 0x7FFFFF00ull,
                   "stem_tconv2d_f16x3_fwd: operand views must stay below 2 GiB (split the batch)");
    int nch[4], maxT = 0;
    Fx3Args a;
    memset(&a, 0, sizeof(a));
    int tapbase = 0;
    for (int p = 0; p < 4; ++p) {
        const TAxis ay = tconv_axis(R, pad, p >> 1), ax = tconv_axis(R, pad, p & 1);
        Fx3Phase &ph = a.ph[p];
        ph.ntaps = ay.cnt * ax.cnt;
        ph.S = ax.cnt;
        ph.dy0 = ay.d0;
        ph.dx0 = ax.d0;
        ph.ooy = p >> 1;
        ph.oox = p & 1;
        ph.wofs = (int)((size_t)ntn * nslab * tapbase * GB_BUF);
        tapbase += ph.ntaps;
        nch[p] = nslab * ph.ntaps;
        maxT = ph.ntaps > maxT ? ph.ntaps : maxT;
        STEM_CHECK_ARG(ph.ntaps >= 1, "stem_tconv2d_f16x3_fwd: empty phase (R=%d)", R);
    }
    // 64-pixel workgroups unless the coarse grid alone fills the chip (HD.2 at B = 16: 34 against 49 us)
    const int forced_bm = stem_tuning(STEM_TUNE_FX3_GEN_TILE);
    const int bm = forced_bm ? forced_bm : (4 * cdiv(M, 128) * ntn >= 256 ? 128 : 64), ptiles = cdiv(M, bm);
    int cps = tconv_cps(ptiles * ntn, nch);
    // the slabs of all phases sit behind each other in ws; without room for the plan the launch is unsplit (same result up to order)
    size_t wsfl = 0;
    int maxns = 1;
    for (int pass = 0; pass < 2; ++pass) {
        wsfl = 0;
        maxns = 1;
        for (int p = 0; p < 4; ++p) {
            Fx3Phase &ph = a.ph[p];
            ph.cps = cps < nch[p] ? cps : nch[p];
            ph.nsplit = cdiv(nch[p], ph.cps);
            ph.wsofs = (int)wsfl;
            if (ph.nsplit > 1) wsfl += (size_t)ph.nsplit * M * ntn * GBN;
            maxns = ph.nsplit > maxns ? ph.nsplit : maxns;
        }
        const bool fits = ws && kGenCntBytes + wsfl * sizeof(float) <= ws_bytes && (size_t)4 * ptiles * ntn * sizeof(int) <= kGenCntBytes &&
                          wsfl * sizeof(float) < 0x7FFFFF00ull;
        if (maxns == 1 || fits) break;
        cps = 1 << 30;                              // second pass: unsplit
    }
    a.xp = xp; a.wp = wp; a.bias = bias; a.y = y; a.yp = yp; a.ldy = ldy; a.z = z; a.ldz = ldz; a.epi = epi; a.slope = slope;
    a.xq = xq; a.yq = yq; a.wq = reinterpret_cast<const float *>(static_cast<const unsigned char *>(wp) + wb);
    a.B = B; a.H = H; a.W = W; a.C = C; a.N = N; a.OH = H; a.OW = W; a.stride = 1;
    a.xbytes = (int)xb; a.wbytes = (int)wb; a.xpix = xpix;
    a.ptiles = ptiles; a.btaps = maxT; a.OHf = OHf; a.OWf = OWf;
    if (maxns > 1) {
        a.cnt = static_cast<int *>(ws);
        a.ws = reinterpret_cast<float *>(static_cast<unsigned char *>(ws) + kGenCntBytes);
    }
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)conv_f16x3_gen_kernel<64, 16, true>, hipFuncAttributeMaxDynamicSharedMemorySize, glds(64));
        (void)hipFuncSetAttribute((const void *)conv_f16x3_gen_kernel<128, 16, true>, hipFuncAttributeMaxDynamicSharedMemorySize, glds(128));
        attr_done = true;
    }
    stem_ran_note(STEM_RAN_TCONV_TILE, bm == 128 ? 128 : 64);      // test aids: stem_tuning_get("tconv_ran_tile" | "tconv_ran_cps" | "tconv_ran_split0" .. "3")
    stem_ran_note(STEM_RAN_TCONV_CPS, cps);
    for (int p = 0; p < 4; ++p) stem_ran_note(STEM_RAN_TCONV_SPLIT0 + p, a.ph[p].nsplit);
    const dim3 grid(4 * ptiles, ntn, maxns);
    if (bm == 128)
        hipLaunchKernelGGL((conv_f16x3_gen_kernel<128, 16, true>), grid, dim3(512), glds(128), (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((conv_f16x3_gen_kernel<64, 16, true>), grid, dim3(256), glds(64), (hipStream_t)stream, a);
    STEM_LAUNCH_CHECK("stem_tconv2d_f16x3_fwd");
    return 0;
}
