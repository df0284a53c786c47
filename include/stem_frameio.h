/* C ABI of the frame ingest / emit kernels of the stand-alone sequence codec (csrc/frameio.hip, libstem_frameio.so): raw planar
 * 4:2:0 frames into, and out of, the zero-padded fp32 RGB frames the image models read and write (video.py).  They are the dense
 * kernels of stem_hip.h (stem_yuv420_to_rgb, stem_rgb_to_yuv420) with the padding / cropping of bitstream.pad / crop folded in:
 * one launch each, and the same bits, because both files take a work item's arithmetic from csrc/yuv_elem.h.  The conventions of
 * stem_hip.h -- device pointers owned by the caller, outputs pre-allocated, asynchronous on `stream`, 0 on success, <0 with the
 * message of stem_frameio_last_error() naming the function otherwise, every argument error reported before any launch.  A header of
 * its own, like stem_gdn1.h: stem_hip.h's list of entry points is the launch tape's table (csrc/tape_entries.inc), and these calls
 * are not part of a recorded training step.  A library of its own as well: libstem_hip.so exports exactly what the other headers
 * declare.  _lib.py reads the ctypes prototypes from here.  stem_abi_version() is unchanged: the entry points are additive.
 *
 * BT.709, full range; peak = 2^bit_depth - 1; samples are 1 or 2 bytes wide, bit_depth 8, or 10 in two bytes.  Both kernels are
 * streaming passes: no atomics, no workspace, no host synchronisation, a repeated call writes the same bits.  Accesses are 16-byte
 * (4-byte for 8-bit samples) vectors where the geometry and the pointers allow it, element by element otherwise.                */
#ifndef STEM_FRAMEIO_H
#define STEM_FRAMEIO_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* y [B][H][W], u and v [B][H/2][W/2] integer planes -> rgb fp32 [B][3][Hp][Wp], dense.  The image occupies rows top .. top + H and
 * columns left .. left + W; every other element of rgb is written +0.0.  The interior is bit for bit what stem_yuv420_to_rgb writes
 * for the same planes (upsample: 0 bilinear, 1 nearest; clamp01): the chroma taps clamp at the image's edge, not the frame's.
 * Refused before launch: H, W odd or < 2, top / left < 0, a window that leaves the frame. */
int stem_yuv420_to_rgb_padded(const void *y, const void *u, const void *v, int B, int H, int W, int sample_bytes, int bit_depth,
                              int upsample, int clamp01, float *rgb, int Hp, int Wp, int top, int left, void *stream);

/* rgb fp32 [B][3][Hp][Wp] with rows row_pitch >= Wp floats apart, colour planes plane_pitch >= (Hp - 1) * row_pitch + Wp floats apart
 * and images 3 * plane_pitch apart (a view of a larger tensor is fine) -> the integer planes yi [B][H][W], ui and vi [B][H/2][W/2] of
 * the window of H x W pixels (both even) at (top, left), dense: bit for bit what stem_rgb_to_yuv420 writes for a dense copy of the
 * window (fp64 evaluation, rint half to even).  top and left may be odd: the 2 x 2 chroma blocks are aligned to the window.  No
 * distortion sums: a decoder has no source. */
int stem_rgb_window_to_yuv420(const float *rgb, int B, int Hp, int Wp, size_t row_pitch, size_t plane_pitch, int top, int left, int H,
                              int W, void *yi, void *ui, void *vi, int sample_bytes, int bit_depth, void *stream);

/* the calling thread's last error message of the two calls above */
const char *stem_frameio_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
