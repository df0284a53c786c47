/* C ABI of the two per-frame device passes of the pixel-domain sequence codec (csrc/roiio.hip, libstem_roiio.so; video_pixel.py):
 * the decoded padded frame becomes the next P frame's condition in place, and a list of rectangles becomes the zero-padded quality
 * map a variable-rate model reads.  The conventions are those of stem_frameio.h -- device pointers owned by the caller, asynchronous
 * on `stream`, 0 on success, <0 with the message of stem_roiio_last_error() naming the function otherwise, every argument error
 * reported before any launch.  A header and a library of their own for the same reasons: stem_hip.h's list of entry points is the
 * launch tape's table, libstem_hip.so and libstem_frameio.so export exactly what their headers declare, and these calls are not part
 * of a recorded training step.  _lib.py reads the ctypes prototypes from here.  stem_abi_version() is unchanged: the entry points are
 * additive.
 *
 * Both kernels are streaming passes: no atomics, no workspace, no host synchronisation, a repeated call writes the same bits.
 * Accesses are 16-byte vectors where the geometry and the pointers allow it, element by element otherwise. */
#ifndef STEM_ROIIO_H
#define STEM_ROIIO_H
#include <stddef.h>
#include <stdint.h>

/* the most rectangles one stem_roi_map_padded call takes (they are staged in LDS once per workgroup) */
#define STEM_ROI_MAX_BOXES 64

#ifdef __cplusplus
extern "C" {
#endif

/* rgb fp32 [B][3][Hp][Wp], pitched as the emit kernel of stem_frameio.h reads it (rows row_pitch >= Wp floats apart, colour planes
 * plane_pitch >= (Hp - 1) * row_pitch + Wp, images 3 * plane_pitch), IN PLACE: the window of H x W pixels (both even) at (top, left)
 * stays as it is, every other element of the logical frame is written +0.0, elements between Wp and row_pitch are not touched.  That
 * is the condition of the next P frame: the cropped reconstruction, zero-padded again.  With yi, ui, vi non-NULL the same pass writes
 * the window's integer 4:2:0 planes yi [B][H][W], ui and vi [B][H/2][W/2], bit for bit those of the emit kernel of stem_frameio.h
 * (both take a work item's arithmetic from csrc/yuv_elem.h).  All three NULL: no planes; one or two NULL is refused.  Every element
 * is either read (window) or written (border), never both, so one launch is safe in place.
 * Refused before launch: what the emit kernel of stem_frameio.h refuses. */
int stem_rgb_window_recondition(float *rgb, int B, int Hp, int Wp, size_t row_pitch, size_t plane_pitch, int top, int left, int H, int W,
                                void *yi, void *ui, void *vi, int sample_bytes, int bit_depth, void *stream);

/* boxes int32 [n][5] = (x0, y0, x1, y1, feather), values fp32 [n], n in 0 .. STEM_ROI_MAX_BOXES -> map fp32 [1][1][Hp][Wp], dense.
 * Rectangles are half-open, in the coordinates of the H x W window at (top, left), and may reach outside it.  Outside the window the
 * map is +0.0.  Window pixel (r, c) starts at v = background; for k = 0 .. n-1 in order, if x0 <= c < x1 and y0 <= r < y1:
 *     d = min(c - x0, x1 - 1 - c, r - y0, y1 - 1 - r)          integers, on the unclipped box
 *     d >= feather:  v = values[k]
 *     otherwise:     t = (float)(d + 1) / (float)(feather + 1);  v = v + (values[k] - v) * t      each operation rounded to fp32
 * Later boxes override earlier ones.  The entry point checks pointers, n and geometry (H, W >= 1; any parity); the contents of the
 * two arrays are device memory and are the caller's to check: x0 < x1, y0 < y1, feather >= 0, values and background in [0, 1]. */
int stem_roi_map_padded(const int32_t *boxes, const float *values, int n, float background, float *map, int Hp, int Wp, int top, int left,
                        int H, int W, void *stream);

/* the calling thread's last error message of the two calls above */
const char *stem_roiio_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
