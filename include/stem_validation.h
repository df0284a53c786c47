/* C ABI of the validation pass's glue kernels (csrc/entropy.hip, part of libstem_hip.so): the eval-mode twins of
 * stem_eb_forward_train / stem_gc_forward_train, and a loss finaliser that keeps a running weighted sum on the device.  With
 * stem_prior_prologue(..., training = 0) they are the elementwise work of one eval-mode P-frame forward plus its EMLoss value
 * (stem/trainSTEM.py:265-295, utils.py:18-27) in 4 launches, and a validation pass over many frames needs ONE device-to-host copy.
 * The conventions of stem_hip.h -- device pointers owned by the caller, outputs pre-allocated, asynchronous on `stream`, 0 on
 * success, <0 with stem_last_error() naming the function otherwise, every argument error reported before any launch.  A header of
 * its own, like stem_gdn1.h: stem_hip.h's list of entry points is the launch tape's table (csrc/tape_entries.inc), and these calls
 * are not part of a recorded training step.  _lib.py reads the ctypes prototypes from here.  stem_abi_version() is unchanged: the
 * entry points are additive.
 *
 * All tensors are fp32 NHWC: npix pixels of C channels.  No kernel here draws noise, and none reads or advances a noise counter.
 *
 * partials: stem_rate_partials(npix * C) doubles (stem_hip.h), one per workgroup of 256 elements: the sum of (double)log2f(lik) over
 * the workgroup's elements by the fixed tree of the training kernels (block_log2_partial) -- every slot is written, no atomics, a
 * repeated call gives the same bits.                                                                                          */
#ifndef STEM_VALIDATION_H
#define STEM_VALIDATION_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* EntropyBottleneck.forward in eval mode with its rate term: z_hat = round(z - median) + median, lik as stem_eb_forward mode 1 --
 * both bit for bit what stem_eb_forward(mode = 1) writes (the same per-channel / per-element form switch at npix <= 4096) -- and
 * the partial sums of log2(lik).  z: pixel pitch ldz >= C floats (a channel slice of a wider buffer is fine); z_hat and lik dense.
 * pack: [C][58] (stem_eb_pack); medians: [C].  npix == 0: 0, nothing is launched. */
int stem_eb_forward_eval_rate(const float *z, int ldz, const float *pack, const float *medians, float *z_hat, float *lik,
                              double *partials, size_t npix, int C, float bound, void *stream);

/* GaussianConditional.forward in eval mode with its rate term: out = round(y - mean) + mean, lik = gauss_lik(|out - mean|, scale)
 * -- both bit for bit what stem_gc_forward(mode = 1) writes -- and the partial sums of log2(lik).  y, out and lik dense; scales and
 * means share the pixel pitch ldsm >= C (the two halves of the parameter network's output).  npix == 0: 0, nothing is launched. */
int stem_gc_forward_eval_rate(const float *y, const float *scales, const float *means, int ldsm, float *out, float *lik,
                              double *partials, size_t npix, int C, float scale_bound, float lik_bound, void *stream);

/* (y_bpp, z_bpp, loss) = (scale * sum partials_y, scale * sum partials_z, y_bpp + z_bpp) exactly as stem_em_loss_finalize computes
 * them (index-order sums, the loss the sum of the two ROUNDED terms), written to out3[3] (may be NULL), and
 *     acc4[0..2] += weight * (y_bpp, z_bpp, loss)        acc4[3] += weight
 * in fp64 (a product rounded, then a sum rounded: no fused multiply-add).  One workgroup, stream-ordered read-modify-write of acc4,
 * no atomics: calls on one stream accumulate in call order; the caller zeroes acc4 first.  A list of 0 partials may be a null
 * pointer.  The weighted mean of a validation pass is acc4[0..2] / acc4[3]. */
int stem_em_loss_accumulate(const double *partials_y, int ny, const double *partials_z, int nz, double scale, double weight,
                            double *out3, double *acc4, void *stream);

#ifdef __cplusplus
}
#endif
#endif
