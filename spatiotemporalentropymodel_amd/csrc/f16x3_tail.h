// The tail of an fp16 convolution kernel -- everything behind its last MFMA -- stated once for conv_f16x3_gen_kernel
// (conv_f16x3.hip) and conv_f16x3_img_kernel (conv_f16x3_img.hip).  What stays in a kernel is the scatter of its accumulators (to
// the split-K workspace or to the LDS tile): that is where the forms differ (ROWL / COLL of the two MFMA shapes against PIXL
// with its rotated column).
//
// Order: partial tile -> workspace, splitk_arrive (stem_common.h), tail_slab_sum -- or, unsplit, accumulators -> LDS tile and back;
// tail_rows, tail_record, the planes pass (the kernel's own loop around planes_store8) with the prologue's tail_oscale.
//
// A kernel uses a piece only where its code from the first to the last MFMA and its register counts come out as with the piece
// written in place (the schedule of the woven loops depends on the whole function):
//   conv_f16x3_gen_kernel: everything but tail_slab_sum (the same loop in its own words: +2 registers through the helper);
//   conv_f16x3_img_kernel: everything; of the output-scale bound only tail_oscale_of (its three maxima share ONE reduction);
//   conv_f16x3_kernel (192 columns): planes_store8 only (tail_record moves code of its fused-GDN section, its bound: registers).
//
// Pieces of a thread.  The epilogue tile is ROWS pixels x GBN channels of fp32 at pitch GTP.  Every pass gives a thread of the NT
// the same 16-byte pieces: column group ec4 = tid & 31, tile rows er0 + ERS k, er0 = tid >> 5, ERS = NT / 32, k < ER = ROWS / ERS.
// Which pixel a tile row is, is the kernel's business: a functor "tile row -> output row, or -1" / the offsets of the pieces.
#pragma once
#include "f16x3_layout.h"

enum { GEN_EPI_BIAS = 0, GEN_EPI_LRELU = 1, GEN_EPI_DACT = 2 };     // Fx3Args::epi / ImgArgs::epi
constexpr int GTP = GBN + 4;                                         // fp32 pitch of the epilogue tile

#ifdef __HIPCC__
// ---- output-scale bound (prologue: its loads and reductions run while the first chunks are in flight) --------------------------
// 2^e of a planes output from an upper bound of |output|; the launch's first workgroup (`first`) leaves 2^-e in the record
__device__ inline float tail_oscale_of(const float bound, float *yq, const bool first)
{
    const int oe = q_exp(bound);
    if (first && threadIdx.x == 0) yq[1] = q_pow2(-oe);
    return q_pow2(oe);
}
// The bound from the operands' maxima: kterms = C * taps products of at most xmax * wmax each, plus the bias (one layer's worth
// of over-estimation: the inputs' maxima are measured).  Every thread of the NT calls it (`red`: >= 16 floats of LDS); 1 without
// planes.  Returned through readfirstlane: it lives across the main loop and stays in a scalar register that way (+2 vector
// registers otherwise).  conv_f16x3_kernel keeps its own statement of this bound, with the fused GDN's factor: see there.
template <int NT>
__device__ inline float tail_oscale(const bool planes, const float *xq, const float *wq, const float *bias, const int N, const int kterms, float *yq,
                                    const bool first, float *red)
{
    float oscale = 1.f;
    if (planes) {
        const float xmax = q_amax(xq, red), wmax = q_amax(wq, red);
        float bm = 0.f;
        if (bias)
            for (int n = threadIdx.x; n < N; n += NT) bm = fmaxf(bm, fabsf(bias[n]));
        bm = block_max(bm, red);
        oscale = tail_oscale_of((float)kterms * xmax * wmax + bm, yq, first);
    }
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, oscale)));
}
// the four bias values of a thread's column group (parameters may sit at any 4-byte offset of a flat buffer: scalar loads)
__device__ inline f32x4 tail_bias4(const float *bias, const int ecol, const int N)
{
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (bias && ecol < N) {              // N % 4 == 0 (host check)
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = bias[ecol + c];
    }
    return b;
}
// ---- owner's slab sum ---------------------------------------------------------------------------------------------------------
// The last arriver sums the nsplit slabs of `slab` floats each in split order, its own included at its place: one fixed order
// whoever arrives last.  eoff[k]: byte offset of the thread's piece k inside a slab, OOR for an absent row.  sc1 16-byte buffer
// loads (device-coherent level, not this XCD's L2), NF pieces x 4 splits in flight: the read is latency-bound (~1 us per dependent
// cross-XCD round).  Absent rows and the splits beyond nsplit are out-of-range loads: zeros.  NF = 8 in the image-tile kernel;
// the general kernel states the same loop itself with NF = 4 (64 registers per round: it keeps its 128), see there.
template <int ER, int NF>
__device__ inline void tail_slab_sum(f32x4 (&ev)[ER], float *ws, const int nsplit, const int slab, const int (&eoff)[ER])
{
    constexpr int SC1 = 16;               // cache-policy bit 4 of the buffer instructions = sc1 on gfx94x / gfx950
    static_assert(ER % NF == 0, "pieces in flight");
    const __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc(ws, 0, (int)((size_t)nsplit * slab * 4), 0x00020000);
    const int sstep = slab * 4;
#pragma unroll
    for (int k = 0; k < ER; ++k) ev[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < ER; kb += NF)
        for (int sp = 0; sp < nsplit; sp += 4) {
            f32x4 tt[NF][4];
#pragma unroll
            for (int k = 0; k < NF; ++k)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    tt[k][u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rws, sp + u < nsplit ? eoff[kb + k] : OOR,
                                                                                                  (sp + u < nsplit ? sp + u : 0) * sstep, SC1));
#pragma unroll
            for (int k = 0; k < NF; ++k)
#pragma unroll
                for (int u = 0; u < 4; ++u) ev[kb + k] += tt[k][u];
        }
}
// ---- epilogue rows ------------------------------------------------------------------------------------------------------------
// v = ev * fac + bias, leaky ReLU or -- DACT -- its derivative selected by z, the 16-byte fp32 row store for the rows that exist
// (orow(tile row) >= 0) and the columns below N; the activated values go back into T when planes are wanted.  Returns this thread's
// max |stored value|.  A thread's four columns are the same in every pass: its bias values come in as `ebias`, and the z rows of
// the DACT epilogue are loaded all at once, before the loop (per-row dependent loads cost ~0.5 us each: 8 us of a 26 us launch).
// `a`: the kernel's arguments (bias-free: N, epi, slope, z, ldz, y, ldy, yp).
template <int ROWS, int NT, typename Args, typename OutRow>
__device__ inline float tail_rows(const Args &a, const f32x4 (&ev)[ROWS / (NT / 32)], float *T, const int ecol, const float fac, const f32x4 ebias,
                                  OutRow &&orow)
{
    constexpr int ERS = NT / 32, ER = ROWS / ERS;
    const int ec4 = threadIdx.x & 31, er0 = threadIdx.x >> 5;
    const bool colok = ecol < a.N;                      // N % 4 == 0 (host check)
    float omax = 0.f;
    f32x4 ez[ER];
    if (a.epi == GEN_EPI_DACT) {
#pragma unroll
        for (int k = 0; k < ER; ++k) {
            const long m = orow(er0 + ERS * k);
            ez[k] = (colok && m >= 0) ? *reinterpret_cast<const f32x4 *>(a.z + m * a.ldz + ecol) : f32x4{1.f, 1.f, 1.f, 1.f};
        }
    }
#pragma unroll
    for (int k = 0; k < ER; ++k) {
        const int row = er0 + ERS * k;
        const long m = orow(row);
        f32x4 v = ev[k] * fac + ebias;
        if (a.epi == GEN_EPI_LRELU) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = v[c] > 0.f ? v[c] : v[c] * a.slope;
        } else if (a.epi == GEN_EPI_DACT) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = ez[k][c] > 0.f ? v[c] : v[c] * a.slope;
        }
        if (colok && m >= 0) {
            if (a.y) *reinterpret_cast<f32x4 *>(a.y + m * a.ldy + ecol) = v;
            omax = fmaxf(fmaxf(omax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        }
        if (a.yp) *reinterpret_cast<f32x4 *>(&T[row * GTP + ec4 * 4]) = v;
    }
    return omax;
}
// ---- scale record -------------------------------------------------------------------------------------------------------------
// max |output| of the workgroup into its slot; the owner of slot 0 writes the header, and inv = 1 without planes (with planes
// tail_oscale_of has left 2^-e there).  Every thread calls it; NT as block_max's.
template <int NT = 0>
__device__ inline void tail_record(float *yq, const bool planes, float omax, float *red, const int slot, const int nslots)
{
    if (!yq) return;
    omax = block_max<NT>(omax, red);
    if (threadIdx.x == 0) {
        yq[QREC_HDR + slot] = omax;
        if (slot == 0) {
            q_header(yq, nslots);
            if (!planes) yq[1] = 1.f;
        }
    }
}
// ---- planes store -------------------------------------------------------------------------------------------------------------
// eight consecutive floats of an LDS tile row (16-byte aligned), times oscale, as the two fp16 pieces of a planes tensor at dst
__device__ inline void planes_store8(const float *t8, const float oscale, unsigned char *dst)
{
    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(t8), v1 = *reinterpret_cast<const f32x4 *>(t8 + 4);
    h16x8 h0, h1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        hp_t x0, x1;
        q_split(v0[c], oscale, x0, x1);
        h0[c] = x0; h1[c] = x1;
        q_split(v1[c], oscale, x0, x1);
        h0[4 + c] = x0; h1[4 + c] = x1;
    }
    *reinterpret_cast<h16x8 *>(dst) = h0;
    *reinterpret_cast<h16x8 *>(dst + PLANE1) = h1;
}
#endif
