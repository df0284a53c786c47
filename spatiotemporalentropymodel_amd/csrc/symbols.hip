// The coding calls of a model without a spatial prior (include/stem_ar_batch.h: stem_symbols_pack, stem_symbols_unpack).  A whole
// frame's symbols go to the host coder in one call, in the reference's flattening order [B][C][H][W]; the latents and their entropy
// parameters live NHWC with a pixel pitch.  One launch states what used to be F.sub + F.round_ + .int() + F.build_indexes + two
// element-wise host transposes (and the mirror on the decoder side).
//
// Both kernels move a tile of TP pixels x TC channels through LDS: the NHWC side is touched in runs of TC consecutive channels
// (256 B per pixel), the NCHW side in runs of TP consecutive pixels (256 B per channel).  The LDS image is [pixel][channel] with a
// row of TC + 1 words: the NHWC phase has a wave's 64 lanes on 64 consecutive words of one row, the NCHW phase has them on one
// column, TC + 1 = 65 words apart, i.e. 1 (mod 32) and 1 (mod 64): conflict-free under either bank modulus of the b32 accesses.
//
// Arithmetic: sym = (int32) rint(y - m) (two fp32 operations, ties to even), y_hat = (float) sym + m (one rounding) and the
// scale-to-index search, all three as ar_canon.h states them.  Compiled without contraction like the products of ar.hip.
#include "ar_canon.h"
#include "../../include/stem_ar_batch.h"

#pragma clang fp contract(off)

namespace {

constexpr int TP = 64;            // pixels per tile
constexpr int TC = 64;            // channels per tile
constexpr int TROW = TC + 1;      // LDS row in words
constexpr int NT = 256;           // threads: 64 lanes along the contiguous side x 4 rows per pass

// grid (ceil(HW / TP), ceil(C / TC), B)
__global__ __launch_bounds__(NT) void symbols_pack_kernel(const float *__restrict__ y, int ldy, const float *__restrict__ means, int ldm,
                                                          const float *__restrict__ chan_means, const float *__restrict__ scales, int lds,
                                                          const float *__restrict__ table, int T, float sb, int32_t *__restrict__ sym,
                                                          int32_t *__restrict__ idx, int HW, int C)
{
    __shared__ int32_t s_sym[TP * TROW];
    __shared__ int32_t s_idx[TP * TROW];
    const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int p0 = blockIdx.x * TP, c0 = blockIdx.y * TC;
    const size_t b = blockIdx.z;
    const bool want_sym = y != nullptr, want_idx = idx != nullptr;

    // NHWC phase: lane = channel, rows of pixels
    const int c = c0 + lane;
    if (c < C) {
        const float cm = chan_means ? chan_means[c] : 0.f;
        for (int pp = row; pp < TP; pp += NT / 64) {
            const int p = p0 + pp;
            if (p >= HW) break;
            const size_t pix = b * (size_t)HW + p;
            if (want_sym) {
                const float v = y[pix * ldy + c];
                float q;
                if (means) quantise(v, means[pix * ldm + c], q);
                else if (chan_means) quantise(v, cm, q);
                else q = round_ties_even(v);                  // no mean: no subtraction
                s_sym[pp * TROW + lane] = (int32_t)q;
            }
            if (want_idx) s_idx[pp * TROW + lane] = scales ? scale_index(scales[pix * lds + c], sb, table, T) : c;
        }
    }
    __syncthreads();
    // NCHW phase: lane = pixel, rows of channels
    const int p = p0 + lane;
    if (p < HW) {
        for (int cc = row; cc < TC; cc += NT / 64) {
            const int ch = c0 + cc;
            if (ch >= C) break;
            const size_t o = (b * (size_t)C + ch) * (size_t)HW + p;
            if (want_sym) sym[o] = s_sym[lane * TROW + cc];
            if (want_idx) idx[o] = s_idx[lane * TROW + cc];
        }
    }
}

__global__ __launch_bounds__(NT) void symbols_unpack_kernel(const int32_t *__restrict__ sym, const float *__restrict__ means, int ldm,
                                                            const float *__restrict__ chan_means, float *__restrict__ y_hat, int ldo,
                                                            int HW, int C)
{
    __shared__ int32_t s_sym[TP * TROW];
    const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int p0 = blockIdx.x * TP, c0 = blockIdx.y * TC;
    const size_t b = blockIdx.z;

    // NCHW phase: lane = pixel, rows of channels
    const int p = p0 + lane;
    if (p < HW) {
        for (int cc = row; cc < TC; cc += NT / 64) {
            const int ch = c0 + cc;
            if (ch >= C) break;
            s_sym[lane * TROW + cc] = sym[(b * (size_t)C + ch) * (size_t)HW + p];
        }
    }
    __syncthreads();
    // NHWC phase: lane = channel, rows of pixels
    const int c = c0 + lane;
    if (c < C) {
        const float cm = chan_means ? chan_means[c] : 0.f;
        for (int pp = row; pp < TP; pp += NT / 64) {
            const int q = p0 + pp;
            if (q >= HW) break;
            const size_t pix = b * (size_t)HW + q;
            const int32_t s = s_sym[pp * TROW + lane];
            y_hat[pix * ldo + c] = means ? dequantise(s, means[pix * ldm + c]) : chan_means ? dequantise(s, cm) : (float)s;      // no mean: no addition
        }
    }
}

inline bool grid_fits(int B, int H, int W, int C)
{
    return (size_t)H * W <= (size_t)0x7FFFFFFF && B <= 65535 && cdiv(C, TC) <= 65535;
}

}   // namespace

STEM_EXPORT int stem_symbols_pack(const float *y, int ldy, const float *means, int ldm, const float *chan_means, const float *scales,
                                  int lds, const float *table, int T, float scale_bound, int32_t *sym, int32_t *idx, int B, int H, int W,
                                  int C, void *stream)
{
    STEM_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "stem_symbols_pack: B, H, W, C must be positive (got %d, %d, %d, %d)", B, H, W, C);
    STEM_CHECK_ARG(grid_fits(B, H, W, C), "stem_symbols_pack: B = %d, H * W = %zu or C = %d exceeds the launch grid", B, (size_t)H * W, C);
    STEM_CHECK_ARG(y || idx, "stem_symbols_pack: neither y (symbols) nor idx (indexes) is given: nothing to write");
    STEM_CHECK_ARG(!y == !sym, "stem_symbols_pack: y and sym are given together or not at all");
    STEM_CHECK_ARG(!(means && chan_means), "stem_symbols_pack: at most one of means and chan_means may be given");
    STEM_CHECK_ARG(y || !(means || chan_means), "stem_symbols_pack: means without y (no symbols are written)");
    STEM_CHECK_ARG(idx || !scales, "stem_symbols_pack: scales without idx (no indexes are written)");
    STEM_CHECK_ARG(!scales || (table && T >= 1), "stem_symbols_pack: scales need a table of T >= 1 entries");
    STEM_CHECK_ARG(!y || ldy >= C, "stem_symbols_pack: ldy = %d is smaller than C = %d", ldy, C);
    STEM_CHECK_ARG(!means || ldm >= C, "stem_symbols_pack: ldm = %d is smaller than C = %d", ldm, C);
    STEM_CHECK_ARG(!scales || lds >= C, "stem_symbols_pack: lds = %d is smaller than C = %d", lds, C);
    const int HW = H * W;
    hipLaunchKernelGGL(symbols_pack_kernel, dim3(cdiv(HW, TP), cdiv(C, TC), B), dim3(NT), 0, (hipStream_t)stream, y, ldy, means, ldm,
                       chan_means, scales, lds, table, T, scale_bound, sym, idx, HW, C);
    STEM_LAUNCH_CHECK("stem_symbols_pack");
    return 0;
}

STEM_EXPORT int stem_symbols_unpack(const int32_t *sym, const float *means, int ldm, const float *chan_means, float *y_hat, int ldo, int B,
                                    int H, int W, int C, void *stream)
{
    STEM_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "stem_symbols_unpack: B, H, W, C must be positive (got %d, %d, %d, %d)", B, H, W, C);
    STEM_CHECK_ARG(grid_fits(B, H, W, C), "stem_symbols_unpack: B = %d, H * W = %zu or C = %d exceeds the launch grid", B, (size_t)H * W, C);
    STEM_CHECK_ARG(sym && y_hat, "stem_symbols_unpack: sym and y_hat must be given");
    STEM_CHECK_ARG(!(means && chan_means), "stem_symbols_unpack: at most one of means and chan_means may be given");
    STEM_CHECK_ARG(!means || ldm >= C, "stem_symbols_unpack: ldm = %d is smaller than C = %d", ldm, C);
    STEM_CHECK_ARG(ldo >= C, "stem_symbols_unpack: ldo = %d is smaller than C = %d", ldo, C);
    const int HW = H * W;
    hipLaunchKernelGGL(symbols_unpack_kernel, dim3(cdiv(HW, TP), cdiv(C, TC), B), dim3(NT), 0, (hipStream_t)stream, sym, means, ldm,
                       chan_means, y_hat, ldo, HW, C);
    STEM_LAUNCH_CHECK("stem_symbols_unpack");
    return 0;
}
