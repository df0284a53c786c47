/*
 * stem_ar_batch.h -- C ABI of libstem_hip.so, continued: raster-order coding of several independent images in one queue, and the
 * wavefront symbol order (a second, opt-in order of the coded symbols in which the decoder advances a step of positions at a time).
 *
 * Same conventions as stem_hip.h (device pointers owned by the caller, asynchronous on `stream`, 0 on success, stem_last_error()
 * on failure).  The entry points here are not launch-tape entries (csrc/tape_entries.inc lists stem_hip.h's): the coding loops
 * are queued by one call each and are not part of a recorded training step.
 *
 * ---- the canonical product ---------------------------------------------------------------------------------------------------
 * Every entropy parameter of the coding loops is specified to the bit: a mean that differs by an ulp moves y_hat and with it every
 * later context, a scale on the other side of a table entry corrupts the stream.  Every product of these loops -- stem_gemv3,
 * stem_gemv3_decode, stem_gemv3_wave, the batched products of stem_ar_encode_batch / stem_ar_decode_batch /
 * stem_ar_decode_wave_batch and the persistent decoder, whose partial sums continue once the symbols arrive -- computes, per output
 * row n, in float32 without fused multiply-add (every product and every sum rounded):
 *   - 64 lane accumulators, 0.0f each;
 *   - the segments in argument order; within a segment lane l takes the columns k = 4l, 4l + 256, ... while k < len, and each step
 *     adds ((x[k] W[n][woff+k] + x[k+1] W[n][woff+k+1]) + x[k+2] W[n][woff+k+2]) + x[k+3] W[n][woff+k+3] to the lane's accumulator;
 *   - the xor butterfly acc += acc[lane ^ off] for off = 32, 16, 8, 4, 2, 1; lane 0's value is the sum;
 *   - y[n] = sum + bias[n] (+ 0.0f without a bias), then v > 0 ? v : v * slope for STEM_ACT_LRELU.
 * The scale-to-index search is T - 1 - #{t < T - 1 : max(scale, scale_bound) <= table[t]}, the quantisation q = rintf(pix - mean)
 * (ties to even), pix <- q + mean, symbol = (int32_t)q; the decoder's pix <- (float)symbol + mean is the same float.
 * csrc/ar_canon.h is the device statement of all of this: the one header in which the kernels' leaf arithmetic is written.
 * tests/ar_ref.py states all of this in numpy and tests/test_hip_ar_ops.py holds every kernel form to it bit for bit.
 */
#ifndef STEM_AR_BATCH_H
#define STEM_AR_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* stem_ar_encode_image (stem_hip.h; spatiotemporalpriors.py:916-961) for G >= 1 independent images of equal H, W, M in lockstep
 * (the GOP chains of evaluation.eval_sequence, the batch elements of compress()): one set of five launches per wavefront step
 * covers the step's positions of all G images, so the launch latency that bounds one image is shared.  Per image every float,
 * symbol and index is that of stem_ar_encode_image (same accumulation order).  buf [G][(H+4)][(W+4)][M]; tp (may be NULL) / hp
 * [G][H*W][2M]; wctx/wh1/wh2/wgp: scratch [G][min(H,(W+2)/3)][2M | n0 | n1 | 2M]; sym/idx [G][H*W][M], raster order per image.
 * All pointers 16-byte aligned, pad == 2, M, n0, n1 and the row lengths multiples of 4. */
int stem_ar_encode_batch(const float *w_ctx, int ld_ctx, const float *b_ctx, const float *w0, int ld0, const float *b0, int n0,
                         const float *w1, int ld1, const float *b1, int n1, const float *w2, int ld2, const float *b2,
                         float *buf, int G, int H, int W, int M, int pad, const float *tp, const float *hp,
                         float *wctx, float *wh1, float *wh2, float *wgp, const float *table, int T, float scale_bound,
                         float slope, int32_t *sym, int32_t *idx, void *stream);

/* ---- wavefront symbol order ------------------------------------------------------------------------------------------------
 * Under the 5x5 type-A mask position (h, w) reads rows h-2 and h-1 at columns w-2 .. w+2 and row h at columns w-2 and w-1, so all
 * positions with equal t = w + 3h are independent of each other.  A stream in WAVEFRONT ORDER holds the symbols of an H x W latent of
 * M channels like this:
 *   - steps run t = 0 .. W + 3(H-1) - 1;
 *   - within a step, rows run h = h0(t) .. h0(t) + np(t) - 1 in ascending order, with w = t - 3h, where
 *     h0(t) = max(0, ceil((t - (W-1)) / 3)) and np(t) = min(H-1, floor(t / 3)) - h0(t) + 1  (wave_range of csrc/ar_canon.h; np(t) = 0 for
 *     the steps between two rows of a latent with W < 3);
 *   - within a position, channels run c = 0 .. M-1.
 * The rank of (h, w, c) is therefore M * (sum over t' < t of np(t')) + (h - h0(t)) * M + c.  codec.wave_order(H, W) states the same
 * order on the host.  Raster order (rank (h * W + w) * M + c) is the reference's and stays the default; a wavefront stream is this
 * project's own format. */

/* sym_raster / idx_raster [G][H*W][M] (what stem_ar_encode_image / stem_ar_encode_batch write) -> sym_wave / idx_wave [G][H*W][M] in
 * wavefront order per image; one launch gathers both tensors.  Device pointers; source and destination must not overlap. */
int stem_ar_to_wave_order(const int32_t *sym_raster, const int32_t *idx_raster, int32_t *sym_wave, int32_t *idx_wave, int G, int H, int W,
                          int M, void *stream);

/* the host symbol decoder of stem_ar_decode_wave_batch: the signature of stem_rans_decoder_decode (include/stem_rans.h), and of
 * stem_symbol_decoder_fn (stem_hip.h) */
typedef int (*stem_wave_symbol_decoder_fn)(void *dec, const int32_t *indexes, size_t n, const int32_t *cdfs, int ncdf, int cdf_stride,
                                           const int32_t *sizes, const int32_t *offsets, int32_t *out);

/* Decoder of wavefront-ordered streams for G >= 1 independent images of equal H, W, M in lockstep: W + 3(H-1) steps instead of the
 * H * W positions of stem_ar_decode_batch.  Step t issues the four products of stem_ar_encode_batch's step t (same kernel, grid and
 * accumulation order: every entropy parameter is the encoder's float), writes the step's CDF indexes to the pinned mailbox, makes ONE
 * stream synchronisation, calls `decode(decs[g], idx_host + g * npmax * M, np(t) * M, ..., sym_host + g * npmax * M)` once per
 * image, and commits y_hat = symbol + mean of the step's positions to buf.  buf [G][(H+4)][(W+4)][M], zero on entry, y_hat on return
 * (the call returns after the stream has drained: the mailboxes are free again); tp (may be NULL) / hp [G][H*W][2M];
 * wctx/wh1/wh2/wgp: scratch [G][npmax][2M | n0 | n1 | 2M] with npmax = min(H,(W+2)/3); idx_host / sym_host: pinned, device-visible
 * [G][npmax][M]; decs[G]: one decoder handle per image.  Device pointers 16-byte aligned, pad == 2, M, n0, n1 and the row lengths
 * multiples of 4. */
int stem_ar_decode_wave_batch(const float *w_ctx, int ld_ctx, const float *b_ctx, const float *w0, int ld0, const float *b0, int n0,
                              const float *w1, int ld1, const float *b1, int n1, const float *w2, int ld2, const float *b2,
                              float *buf, int G, int H, int W, int M, int pad, const float *tp, const float *hp,
                              float *wctx, float *wh1, float *wh2, float *wgp, const float *table, int T, float scale_bound, float slope,
                              int32_t *idx_host, int32_t *sym_host, stem_wave_symbol_decoder_fn decode, void *const *decs,
                              const int32_t *cdfs, int ncdf, int cdf_stride, const int32_t *sizes, const int32_t *offsets, void *stream);

/* ---- one-shot coding calls ----------------------------------------------------------------------------------------------------
 * A model without a spatial prior codes a whole frame's symbols in one host call.  These two launches are the device side of that
 * call: y, means, scales and y_hat are NHWC with a pixel pitch (ld >= C; the channel slices of an entropy-parameter output go in
 * as they are), sym and idx are dense [B][C][H][W], the order in which the reference flattens and stem_rans_encode /
 * stem_rans_decode read.  The transpose goes through an LDS tile of 64 pixels x 64 channels.  No atomics, no workspace. */

/* sym = (int32_t)rintf(y - m) with m = means[b,h,w,c], else chan_means[c] (a bottleneck's medians), else sym = (int32_t)rintf(y):
 * the subtraction and the rounding (ties to even) are two fp32 operations, never contracted.  idx = the scale-to-index search
 * T - 1 - #{t < T - 1 : max(scales[b,h,w,c], scale_bound) <= table[t]}; with scales == NULL idx = c (the bottleneck's indexes; table
 * and T are not read).  y == NULL (then sym == NULL, and no means) writes only idx: the decoder's call.  idx == NULL (then no scales)
 * writes only sym.  At most one of means / chan_means.  Null or contradictory arguments, a pitch below C and non-positive sizes
 * return non-zero before any launch. */
int stem_symbols_pack(const float *y, int ldy, const float *means, int ldm, const float *chan_means,
                      const float *scales, int lds, const float *table, int T, float scale_bound,
                      int32_t *sym, int32_t *idx, int B, int H, int W, int C, void *stream);

/* y_hat[b,h,w,c] = (float)sym[b][c][h][w] + m, one rounding (m as above; without means the converted symbol itself). */
int stem_symbols_unpack(const int32_t *sym, const float *means, int ldm, const float *chan_means,
                        float *y_hat, int ldo, int B, int H, int W, int C, void *stream);

#ifdef __cplusplus
}
#endif
#endif
