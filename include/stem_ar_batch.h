/*
 * stem_ar_batch.h -- C ABI of libstem_hip.so, continued: raster-order coding of several independent images in one queue.
 *
 * Same conventions as stem_hip.h (device pointers owned by the caller, asynchronous on `stream`, 0 on success, stem_last_error()
 * on failure).  The entry points here are not launch-tape entries (csrc/tape_entries.inc lists stem_hip.h's): the coding loops
 * are queued by one call each and are not part of a recorded training step.
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

#ifdef __cplusplus
}
#endif
#endif
