"""The numpy float32 statement of the ROI rasteriser (include/stem_roiio.h: stem_roi_map_padded), operation by operation in the stated
order.  tests/test_roi_map_ref.py pins it against a plain per-pixel loop; the GPU tests compare the kernel with it bit for bit."""
import numpy as np


def roi_map(boxes, size, background=0.0):
    """boxes: (x0, y0, x1, y1, value[, feather]) in order -> the map [h, w] float32 of the h x w window"""
    h, w = size
    f32 = np.float32
    out = np.full((h, w), f32(background), dtype=np.float32)
    for box in boxes:
        x0, y0, x1, y1 = (int(a) for a in box[:4])
        value, feather = f32(box[4]), int(box[5]) if len(box) > 5 else 0
        ra, rb, ca, cb = max(y0, 0), min(y1, h), max(x0, 0), min(x1, w)
        if ra >= rb or ca >= cb:
            continue                                                                  # no window pixel inside: contributes nothing
        r, c = np.arange(ra, rb, dtype=np.int64)[:, None], np.arange(ca, cb, dtype=np.int64)[None, :]
        d = np.minimum(np.minimum(c - x0, x1 - 1 - c), np.minimum(r - y0, y1 - 1 - r))   # integers, on the unclipped box
        t = (d + 1).astype(np.float32) / f32(feather + 1)                             # float32 arrays: every operation below rounds to fp32
        v = out[ra:rb, ca:cb]
        diff = value - v
        prod = diff * t
        blended = v + prod
        assert diff.dtype == prod.dtype == blended.dtype == t.dtype == np.float32
        out[ra:rb, ca:cb] = np.where(d >= feather, value, blended)
    return out


def roi_map_padded(boxes, size, background=0.0, multiple=64, frame=None):
    """-> [1, 1, Hp, Wp] float32: `roi_map` at (top, left) of a zero frame (bitstream.pad's centred geometry unless frame=(Hp, Wp, top, left))"""
    h, w = size
    if frame is None:
        Hp, Wp = (h + multiple - 1) // multiple * multiple, (w + multiple - 1) // multiple * multiple
        top, left = (Hp - h) // 2, (Wp - w) // 2
    else:
        Hp, Wp, top, left = frame
    out = np.zeros((1, 1, Hp, Wp), dtype=np.float32)
    out[0, 0, top:top + h, left:left + w] = roi_map(boxes, size, background)
    return out


#: the cases of the CPU test, reused on the GPU: name -> (boxes, (h, w), background).  Dyadic values and feather + 1 a power of two:
#: every intermediate is exactly representable, so float64 and float32 agree to the bit.
EXACT_CASES = {
    "no boxes": ([], (6, 10), 0.25),
    "one box, no feather": ([(2, 1, 7, 5, 0.75)], (6, 10), 0.25),
    "feather 0 given": ([(2, 1, 7, 5, 0.75, 0)], (6, 10), 0.25),
    "feather 1": ([(1, 1, 9, 6, 1.0, 1)], (8, 12), 0.0),
    "feather 3": ([(2, 2, 20, 18, 0.5, 3)], (20, 24), 0.125),
    "feather larger than half the box": ([(3, 2, 9, 6, 0.75, 7)], (10, 12), 0.25),
    "later boxes override": ([(0, 0, 8, 8, 0.5), (4, 4, 12, 12, 1.0), (6, 0, 10, 6, 0.25)], (12, 12), 0.0),
    "override with feather over a box": ([(0, 0, 12, 12, 1.0), (2, 2, 10, 10, 0.0, 3)], (12, 12), 0.5),
    "clipped by the window": ([(-3, -2, 5, 4, 0.75, 1), (8, 5, 40, 30, 0.5, 3)], (8, 12), 0.25),
    "wholly outside": ([(20, 20, 30, 30, 1.0), (-9, 0, -1, 4, 1.0, 1)], (8, 12), 0.25),
    "value below background": ([(2, 2, 10, 8, 0.125, 1)], (10, 12), 0.875),
}
