/* C ABI of the block kernels of the cheng2020 I-frame models (csrc/resblock.hip, part of libstem_hip.so): the conventions of
 * stem_hip.h -- device pointers owned by the caller, outputs pre-allocated, asynchronous on `stream`, 0 on success, <0 with
 * stem_last_error() naming the function otherwise.  A header of its own, like stem_ar_batch.h: stem_hip.h's list of entry points is
 * the launch tape's table (csrc/tape_entries.inc), and these calls are not part of a recorded training step.  _lib.py reads the
 * ctypes prototypes from here.  stem_abi_version() is unchanged: the entry points are additive. */
#ifndef STEM_BLOCKS_H
#define STEM_BLOCKS_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- residual / sub-pixel / attention blocks (compressai/layers/layers.py:50-213) ----
 * fp32 NHWC, one pixel pitch (`ld*`, in floats) per tensor so that channel-slice views need no copy.  Where the channel count of
 * a tensor is a multiple of 4 it is accessed 16 bytes at a time: its pitch is then a multiple of 4 and its base 16-byte aligned
 * (anything else is an argument error).  act = LeakyReLU(slope): slope 1 = identity, slope 0 = ReLU.  Results are stated bit for
 * bit (single roundings, no FMA contraction) except the gate's, which goes through expf.
 *
 * nn.PixelShuffle(r) (compressai/layers/layers.py:55-59: subpel_conv3x3) with what follows it in ResidualBlockUpsample
 * (layers.py:118-126: leaky_relu; `out += identity`) folded in:  in [B,H,W,C*r*r], out / addend [B,H*r,W*r,C],
 *   out[b, h*r+i, w*r+j, c] = act(in[b, h, w, c*r*r + i*r + j]) (+ addend[b, h*r+i, w*r+j, c]);   addend may be NULL.        */
int stem_pixel_shuffle_fwd(const float *in, int ldi, const float *addend, int lda, float *out, int ldo, int B, int H, int W, int C,
                           int r, float slope, void *stream);
/* its adjoint: din[b, h, w, c*r*r + i*r + j] = dout[b, h*r+i, w*r+j, c] * (in > 0 ? 1 : slope); `in` (the forward input) may be
 * NULL when slope == 1.  The addend's gradient is dout itself.                                                                */
int stem_pixel_shuffle_bwd(const float *in, int ldi, const float *dout, int ldo, float *din, int ldd, int B, int H, int W, int C,
                           int r, float slope, void *stream);
/* ResidualUnit's relu(conv(x) + identity) (layers.py:191-196): out = act(a + b) over npix pixels of C channels;
 * backward: da = db = dab = dout * (out > 0 ? 1 : slope)                                                                     */
int stem_add_act_fwd(const float *a, int lda, const float *b, int ldb, float *out, int ldo, size_t npix, int C, float slope, void *stream);
int stem_add_act_bwd(const float *out, int ldo, const float *dout, int ldd, float *dab, int ldg, size_t npix, int C, float slope,
                     void *stream);
/* AttentionBlock.forward (layers.py:207-213): out = a * sigmoid(b) + x;  backward, with s = sigmoid(b) recomputed:
 * da = dout * s, db = dout * a * s * (1 - s); dx is dout itself                                                              */
int stem_gate_fwd(const float *a, int lda, const float *b, int ldb, const float *x, int ldx, float *out, int ldo, size_t npix, int C,
                  void *stream);
int stem_gate_bwd(const float *a, int lda, const float *b, int ldb, const float *dout, int ldd, float *da, int ldda, float *db, int lddb,
                  size_t npix, int C, void *stream);

#ifdef __cplusplus
}
#endif
#endif
