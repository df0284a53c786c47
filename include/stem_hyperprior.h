/* C ABI of the zero-mean likelihood kernels of the bmshj2018 I-frame models (csrc/hyperprior.hip, part of libstem_hip.so): the
 * conventions of stem_hip.h -- device pointers owned by the caller, outputs pre-allocated, asynchronous on `stream`, 0 on success,
 * <0 with stem_last_error() naming the function otherwise.  A header of its own, like stem_blocks.h: stem_hip.h's list of entry
 * points is the launch tape's table (csrc/tape_entries.inc), and these calls are not part of a recorded training step.  _lib.py
 * reads the ctypes prototypes from here.  stem_abi_version() is unchanged: the entry points are additive. */
#ifndef STEM_HYPERPRIOR_H
#define STEM_HYPERPRIOR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* All tensors fp32 NHWC, npix pixels of C channels, one pixel pitch (`ld*`, in floats, >= C) per tensor so that channel-slice
 * views need no copy.  Where C and every pitch of a call are multiples of 4 and every base is 16-byte aligned the tensors are
 * accessed 16 bytes at a time, one float at a time otherwise: the results do not depend on which.  npix == 0: 0, nothing launched.
 *
 * GaussianConditional.forward(inputs, scales, means=None) (compressai/entropy_models/entropy_models.py:570-596) in one launch:
 *   mode 0 (training): out = y + n, n = noise[..] when `noise` is given, else the U(-1/2, 1/2) draw of the Philox stream at
 *                      (seed, offset [+ epoch_dev[0] * epoch_stride]) and logical element index pix * C + c: the value
 *                      stem_uniform_noise(_epoch) writes there, bit for bit
 *   mode 1 (eval):     out = rintf(y): no mean is subtracted or added, so a -0.0 keeps its sign
 *   lik = max(Phi((0.5 - |out|) / s) - Phi((-0.5 - |out|) / s), lik_bound),  s = max(scales, scale_bound)
 * Equal (==) element by element to stem_gc_forward fed a tensor of zeros as `means`.                                          */
int stem_gc_scale_forward(const float *y, int ldy, const float *noise, int ldn, uint64_t seed, uint64_t offset,
                          const long long *epoch_dev, uint64_t epoch_stride, const float *scales, int lds, float *out, int ldo,
                          float *lik, int ldl, size_t npix, int C, int mode, float scale_bound, float lik_bound, void *stream);
/* its backward, stem_gc_backward without d means: `out`, `scales` as the forward had them, dlik = d loss / d lik;
 *   dscales (optional) with the LowerBound rule of the scale;  dy (optional) = dv * sign(out) (+ dout where `dout`, the gradient
 *   that arrived at `out`, is given: one fp32 addition);  q (optional): the scale record of (dscales | dv), one slot of max |value|
 *   per 256 logical elements (16 + ceil(npix * C / 256) floats, stem_hip.h: stem_qrec), the record stem_gc_backward writes.
 * Bit-identical to stem_gc_backward fed zeros as `means`, followed by stem_add(dy, dout).                                     */
int stem_gc_scale_backward(const float *out, int ldo, const float *scales, int lds, const float *dlik, int ldl, const float *dout,
                           int ldg, float *dscales, int ldds, float *dy, int lddy, size_t npix, int C, float scale_bound,
                           float lik_bound, float *q, void *stream);
/* ScaleHyperprior's h_a(|y|) (compressai/models/priors.py:258): out = |x|;  dx = g * sign(x) with sign(+-0) = 0 (torch.abs)   */
int stem_abs_fwd(const float *x, int ldx, float *out, int ldo, size_t npix, int C, void *stream);
int stem_abs_bwd(const float *x, int ldx, const float *g, int ldg, float *dx, int lddx, size_t npix, int C, void *stream);

#ifdef __cplusplus
}
#endif
#endif
