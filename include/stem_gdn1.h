/* C ABI of the GDN1 kernels (csrc/gdn1.hip, part of libstem_hip.so): the simplified normalisation of compressai/layers/gdn.py:70-96,
 * y = x / (beta' + gamma' |x|) (inverse: y = x (beta' + gamma' |x|)), forward and backward.  The conventions of stem_hip.h -- device
 * pointers owned by the caller, outputs pre-allocated, asynchronous on `stream`, 0 on success, <0 with stem_last_error() naming the
 * function otherwise, every argument error reported before any launch.  A header of its own, like stem_hyperprior.h and
 * stem_eb_filters.h: stem_hip.h's list of entry points is the launch tape's table (csrc/tape_entries.inc), and these calls are not part
 * of a recorded training step.  _lib.py reads the ctypes prototypes from here.  stem_abi_version() is unchanged: the entry points are
 * additive.
 *
 * All tensors are fp32 NHWC: npix pixels of C channels, pixel pitch ld* >= C floats (channel-slice views of wider buffers are fine).
 * beta[C] and gamma[C][C] are the STORED parameters (row i of gamma = output channel i, the reference's gamma.reshape(C, C, 1, 1)):
 *     beta'[i]     = max(beta[i], sqrt(beta_min + 2^-36))^2 - 2^-36             (ops/parametrizers.py:42-45)
 *     gamma'[i][j] = max(gamma[i][j], 2^-18)^2 - 2^-36
 *     n[p][i]      = beta'[i] + sum_j gamma'[i][j] |x[p][j]|
 * The sum is an fp32 matrix-instruction chain in ascending j that starts at 0; beta' is added last.  A pixel's result depends on
 * nothing but that pixel: not on its position, its neighbours, a pitch, an alignment or the access width the kernel picked (16 bytes
 * where C, every pitch and every base allow it, 4 bytes otherwise).  No |x| and no gamma' tensor exists in memory.
 *
 * npix == 0: 0, nothing is launched, nothing else is looked at.                                                                 */
#ifndef STEM_GDN1_H
#define STEM_GDN1_H
#include <stddef.h>
#include <stdint.h>

#define STEM_GDN1_MAX_C 320          /* a larger C is refused (the backward's three pixel tiles and the gamma chunk fill the LDS) */
#define STEM_GDN1_PIX_CHUNK 1024     /* pixels per partial of the parameter reduction: chunk c covers pixels [c, c + 1) * 1024 */

#ifdef __cplusplus
extern "C" {
#endif

/* y = x * (1 / n) (inverse != 0: y = x * n).  One launch, no scratch. */
int stem_gdn1_fwd(const float *x, int ldx, const float *beta, const float *gamma, float *y, int ldy, size_t npix, int C, int inverse,
                  float beta_min, void *stream);
/* bytes of stem_gdn1_bwd's workspace: g[npix][C] and one [C][C] + [C] partial per STEM_GDN1_PIX_CHUNK pixels.  Host arithmetic only;
 * 0 for npix == 0 or C outside 1 .. STEM_GDN1_MAX_C; monotone in npix. */
size_t stem_gdn1_bwd_workspace_bytes(size_t npix, int C);
/* given dy = d loss / d y:
 *     forward:  r = 1 / n;  u = dy r;  g = -dy x r^2             inverse:  u = dy n;  g = dy x
 *     dx[p][j]      = u[p][j] + sgn(x[p][j]) sum_i g[p][i] gamma'[i][j]          sgn(+-0) = 0 (torch.abs; as stem_abs_bwd)
 *     dgamma'[i][j] = sum_p g[p][i] |x[p][j]|        dbeta'[i] = sum_p g[p][i]
 *     d stored      = 2 max(v, bound) d', passed iff v >= bound or d' < 0        (ops/bound_ops.py:28-31)
 * dx may be NULL; dbeta and dgamma may be NULL together; all three NULL is an argument error.  ws (16-byte aligned, ws_bytes >=
 * stem_gdn1_bwd_workspace_bytes) is needed for dbeta / dgamma only and may be NULL without them.
 * Launches: one per pixel tile for dx and g; one for the partials (pixels of a chunk in ascending order); one that sums the partials
 * in chunk order and applies the reparametrisation rule.  No atomics, every workspace word is written before it is read: a repeated
 * call gives the same bits, whatever the workspace held. */
int stem_gdn1_bwd(const float *x, int ldx, const float *dy, int lddy, const float *beta, const float *gamma, float *dx, int lddx,
                  float *dbeta, float *dgamma, size_t npix, int C, int inverse, float beta_min, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
