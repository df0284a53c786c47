"""CPU: tests/roi_map_ref.py, the numpy float32 statement of the ROI rasteriser the GPU tests compare the kernel with, against a plain
per-pixel loop in float64 written from the definition in include/stem_roiio.h.  The inputs make every intermediate exactly representable
(dyadic values, feather + 1 a power of two), so the two agree to the bit and no tolerance is needed."""
import numpy as np
import pytest

import roi_map_ref


def _loop64(boxes, size, background):
    h, w = size
    out = np.empty((h, w), dtype=np.float64)
    for r in range(h):
        for c in range(w):
            v = float(background)
            for box in boxes:
                x0, y0, x1, y1, value = box[:5]
                feather = box[5] if len(box) > 5 else 0
                if x0 <= c < x1 and y0 <= r < y1:
                    d = min(c - x0, x1 - 1 - c, r - y0, y1 - 1 - r)
                    if d >= feather:
                        v = float(value)
                    else:
                        v = v + (float(value) - v) * ((d + 1) / (feather + 1))
            out[r, c] = v
    return out


@pytest.mark.parametrize("name", list(roi_map_ref.EXACT_CASES))
def test_the_reference_is_the_definition(name):
    boxes, size, background = roi_map_ref.EXACT_CASES[name]
    got = roi_map_ref.roi_map(boxes, size, background)
    want = _loop64(boxes, size, background)
    assert got.dtype == np.float32 and got.shape == tuple(size)
    assert np.array_equal(got.astype(np.float64), want), name


def test_the_pinned_properties():
    m = roi_map_ref.roi_map
    assert np.array_equal(m([], (4, 6), 0.25), np.full((4, 6), 0.25, np.float32))                                  # n = 0: the background
    a = m([(0, 0, 8, 8, 0.5), (4, 4, 12, 12, 1.0)], (12, 12), 0.0)                                                  # later boxes override
    assert a[3, 3] == 0.5 and a[5, 5] == 1.0 and a[11, 11] == 1.0 and a[0, 11] == 0.0
    b = m([(4, 4, 12, 12, 1.0), (0, 0, 8, 8, 0.5)], (12, 12), 0.0)
    assert b[5, 5] == 0.5 and b[9, 9] == 1.0
    c = m([(-3, -2, 5, 4, 0.75, 1)], (8, 12), 0.25)                                                                  # clipped: d on the unclipped box
    assert c[0, 0] == 0.75 and c[3, 0] == 0.5 and c[0, 4] == 0.5 and c[4, 0] == 0.25 and c[0, 5] == 0.25
    assert np.array_equal(m([(20, 20, 30, 30, 1.0), (-9, 0, -1, 4, 1.0, 1)], (8, 12), 0.25), np.full((8, 12), 0.25, np.float32))
    assert np.array_equal(m([(2, 1, 7, 5, 0.75, 0)], (6, 10), 0.25), m([(2, 1, 7, 5, 0.75)], (6, 10), 0.25))        # feather 0: a hard edge
    d = m([(3, 2, 9, 6, 0.75, 7)], (10, 12), 0.25)                                                                   # feather > half the box
    assert d.max() == np.float32(0.25 + 0.5 * 2 / 8) and d[2, 3] == np.float32(0.25 + 0.5 / 8)                       # never reaches the value
    e = m([(2, 2, 10, 8, 0.125, 1)], (10, 12), 0.875)                                                                # value below background
    assert e[2, 2] == 0.5 and e[4, 5] == 0.125 and e[0, 0] == 0.875


def test_the_padded_form_is_bitstream_pad():
    import torch
    from spatiotemporalentropymodel_amd import bitstream
    boxes, size, background = roi_map_ref.EXACT_CASES["clipped by the window"]
    want = bitstream.pad(torch.from_numpy(roi_map_ref.roi_map(boxes, size, background)).reshape(1, 1, *size), 64).numpy()
    got = roi_map_ref.roi_map_padded(boxes, size, background)
    assert got.shape == (1, 1, 64, 64) and np.array_equal(got, want)
    placed = roi_map_ref.roi_map_padded(boxes, size, background, frame=(13, 17, 2, 3))
    assert placed.shape == (1, 1, 13, 17) and np.array_equal(placed[0, 0, 2:10, 3:15], roi_map_ref.roi_map(boxes, size, background))
    assert placed.sum() == roi_map_ref.roi_map(boxes, size, background).sum()
