/* C ABI of the EntropyBottleneck kernels for any `filters` tuple (csrc/eb_filters.hip, part of libstem_hip.so): the conventions of
 * stem_hip.h -- device pointers owned by the caller, outputs pre-allocated, asynchronous on `stream`, 0 on success, <0 with
 * stem_last_error() naming the function otherwise.  A header of its own, like stem_blocks.h and stem_hyperprior.h: stem_hip.h's
 * list of entry points is the launch tape's table (csrc/tape_entries.inc), and these calls are not part of a recorded training
 * step.  _lib.py reads the ctypes prototypes from here.  stem_abi_version() is unchanged: the entry points are additive.
 *
 * The density of a channel is the network 1 -> filters[0] -> ... -> filters[n-1] -> 1 of the reference
 * (compressai/entropy_models/entropy_models.py:294-335, 388-407): widths = (1, *filters, 1), L = n_filters, layers i = 0 .. L,
 * layer i maps widths[i] -> widths[i+1]; every layer but the last has a gate `x += tanh(factor) * tanh(x)`.  stem_eb_* (stem_hip.h)
 * is this family specialised for filters = (3, 3, 3, 3).
 *
 * `filters` is HOST memory (n_filters ints; may be NULL when n_filters == 0).  Every entry point returns -1 before any launch for
 * n_filters outside 0 .. STEM_EBF_MAX_FILTERS, a width outside 1 .. STEM_EBF_MAX_WIDTH, a null pointer where one is required, and
 * C <= 0.
 *
 * Pack layout, [C][nparam] floats, per channel and in this order for i = 0 .. L:
 *     matrix_i   widths[i+1] x widths[i], row major (row = output)
 *     bias_i     widths[i+1]
 *     factor_i   widths[i+1]                 (i < L only)
 * nparam = sum of these; for (3, 3, 3, 3) it is stem_eb_pack's [C][58] image, offset for offset.                              */
#ifndef STEM_EB_FILTERS_H
#define STEM_EB_FILTERS_H
#include <stddef.h>
#include <stdint.h>

#define STEM_EBF_MAX_FILTERS 6     /* at most 7 layers */
#define STEM_EBF_MAX_WIDTH 8
#define STEM_EBF_MAX_NPARAM 433    /* floats per channel at (8, 8, 8, 8, 8, 8) */

#ifdef __cplusplus
extern "C" {
#endif

/* floats per channel of the pack; -1 outside the caps.  Host arithmetic only: no device, no error string */
int stem_ebf_nparam(const int *filters, int n_filters);
/* `tensors`: host array of the 3 L + 2 device pointers matrix_0, bias_0, factor_0, matrix_1, ..., matrix_L, bias_L, each tensor
 * dense [C][its length per channel]  ->  pack[C][nparam] */
int stem_ebf_pack(const float *const *tensors, const int *filters, int n_filters, float *pack, int C, void *stream);
/* dpack[C][nparam] -> the 3 L + 2 gradient tensors (same order and shapes); accumulate != 0 adds (one fp32 addition each) */
int stem_ebf_unpack_grads(const float *dpack, float *const *tensors, const int *filters, int n_filters, int C, int accumulate,
                          void *stream);
/* EntropyBottleneck.forward (entropy_models.py:424-452), stem_eb_forward's contract: z is NHWC with pixel pitch ldz >= C, noise,
 * z_hat and lik are dense [B][H][W][C].
 *   mode 0: z_hat = z + noise (one fp32 addition);   mode 1: z_hat = rintf(z - medians[c]) + medians[c]
 *   lo = logits(z_hat - 1/2), up = logits(z_hat + 1/2), s = -sign(lo + up), lik = max(|sigmoid(s up) - sigmoid(s lo)|, bound)
 * The transformed parameters (softplus of the matrices, tanh of the factors) are computed once per workgroup.                 */
int stem_ebf_forward(const float *z, int ldz, const float *noise, const float *pack, const float *medians, const int *filters,
                     int n_filters, float *z_hat, float *lik, int B, int H, int W, int C, int mode, float bound, void *stream);
/* its backward, stem_eb_backward's contract: dlik = d loss / d lik (dense) reaches the network only where
 * |sigmoid(s up) - sigmoid(s lo)| >= bound or dlik < 0 (LowerBound, ops/bound_ops.py:28-31).
 *   dz (optional, dense) = d loss / d z (+ dzhat_in where given: one fp32 addition);   dpack (optional) [C][nparam], written.
 * One workgroup per channel; sums over pixels in a fixed order, no atomics: two launches give the same bits, and a channel's row
 * does not depend on the other channels.  No workspace.                                                                       */
int stem_ebf_backward(const float *z_hat, const float *pack, const float *dlik, const float *dzhat_in, const int *filters,
                      int n_filters, float *dz, float *dpack, int B, int H, int W, int C, float bound, void *stream);
/* EntropyBottleneck.loss (entropy_models.py:383-386), stem_eb_aux_loss_grad's contract: loss[0] = sum over channels and the three
 * quantiles of |logits(quantiles[c][q]) - target3[q]| is WRITTEN (one fixed-order sum, nothing to zero beforehand);
 * dquantiles (optional) [C][3] is written, or added to when accumulate != 0.  One workgroup walks the channels in chunks: its LDS
 * does not depend on C.                                                                                                        */
int stem_ebf_aux_loss_grad(const float *quantiles, const float *pack, const float *target3, const int *filters, int n_filters,
                           float *loss, float *dquantiles, int C, int accumulate, void *stream);

#ifdef __cplusplus
}
#endif
#endif
