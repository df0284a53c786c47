/* C ABI of the conditioning-state hash of the two sequence codecs (csrc/statehash.hip, libstem_statehash.so; video.py, video_pixel.py):
 * 64 bits per image over the exact fp32 state the next P frame is conditioned on, computed on the device, written into the file by
 * the encoder and compared by the decoder after every frame.  The conventions are those of stem_roiio.h -- device pointers owned by
 * the caller, asynchronous on `stream`, 0 on success, <0 with the message of stem_statehash_last_error() naming the function otherwise,
 * every argument error reported before any launch.  A header and a library of their own for the same reasons: stem_hip.h's list of
 * entry points is the launch tape's table, the other libraries export exactly what their headers declare, and this call is not part
 * of a recorded training step.  _lib.py reads the ctypes prototypes from here.  stem_abi_version() is unchanged: the entry points are
 * additive.
 *
 * Definition (tests/state_hash_ref.py restates it in numpy).  For image b of x [B][C][H][W]:
 *
 *     out[b] = sum over (c, h, w) of mix64((i << 32) | bits(x[b,c,h,w]))   mod 2^64
 *
 * with i = (c * H + h) * W + w the LOGICAL NCHW index, bits the float's 32-bit pattern, and mix64 the SplitMix64 output function
 *
 *     z = k + 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31
 *
 * all mod 2^64.  The index is logical, so the hash is a function of the values and not of the memory layout; the terms are added as
 * integers, so every split over lanes, wavefronts and workgroups gives the same 64 bits; +0.0 and -0.0, and two NaN payloads, hash
 * differently: the state is its bits. */
#ifndef STEM_STATEHASH_H
#define STEM_STATEHASH_H
#include <stddef.h>
#include <stdint.h>

/* elements one workgroup consumes (in memory order along the unit-stride dimension) */
#define STEM_STATE_HASH_CHUNK 4096

#ifdef __cplusplus
extern "C" {
#endif

/* x fp32 [B][C][H][W] with strides sb, sc, sh, sw in floats -> out [B] (8-byte aligned).  Two layouts, both possibly pitched:
 *     channels-last   sc == 1, sw >= C, sh >= (W - 1) * sw + C        images sb >= (H - 1) * sh + (W - 1) * sw + C apart
 *     planar          sw == 1, sh >= W, sc >= (H - 1) * sh + W        images sb >= (C - 1) * sc + (H - 1) * sh + W apart
 * (sb is not looked at when B == 1).  Elements in the gaps of a pitched view are not read.  A streaming pass: every workgroup of the
 * first launch hashes STEM_STATE_HASH_CHUNK elements into one partial sum in `workspace`, a second launch of one workgroup per image
 * adds an image's partials into out[b]; an image of at most one chunk goes straight to out[b] in one launch and needs no workspace.
 * Every word the second launch reads was written by the first, so the workspace's earlier contents do not matter, nothing is zeroed,
 * and a repeated call writes the same bits.  16-byte loads where C (W), the pitches and the pointer allow it.  No host synchronisation.
 * Refused before launch: a null x or out, a null workspace where stem_state_hash_workspace_bytes() is not 0, workspace_bytes below it,
 * B, C, H, W < 1, B > 65535, C * H * W > 2^32, every other stride pattern (a stride of 2^40 or more included), x not 4-byte or out and
 * workspace not 8-byte aligned. */
int stem_state_hash(const float *x, int B, int C, int H, int W, size_t sb, size_t sc, size_t sh, size_t sw, uint64_t *out, void *workspace,
                    size_t workspace_bytes, void *stream);

/* bytes of workspace a stem_state_hash call of that geometry needs: 0 for images of at most one chunk (and for a geometry the call
 * refuses), B * ceil(C * H * W / STEM_STATE_HASH_CHUNK) * 8 otherwise */
size_t stem_state_hash_workspace_bytes(int B, int C, int H, int W);

/* the calling thread's last error message of stem_state_hash */
const char *stem_statehash_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
