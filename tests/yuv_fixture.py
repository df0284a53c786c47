"""Loader of tests/golden/yuv_transforms*.npz (written by tests/golden/make_golden_yuv.py, which is not part of the test run) for
tests/test_yuv_abi.py and tests/test_hip_yuv.py.  Members are named "<case>/<name>/<image>"; inputs (y, u, v, src) exist for every
image of a case, float results for the images listed in "<case>/ref_images" (all of them for the small shapes, the last one
otherwise), float32 results only for the shapes up to 34x70."""
import glob
import os

import numpy as np

from conftest import GOLDEN


def load():
    """{ "<case>/<name>": array stacked over the images stored, in image order }"""
    parts = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "yuv_transforms*.npz"))):
        with np.load(path, allow_pickle=False) as z:
            for k in z.files:
                case, name, b = k.split("/")
                parts.setdefault(f"{case}/{name}", {})[int(b)] = z[k]
    out = {k: np.stack([v[b] for b in sorted(v)]) for k, v in parts.items()}
    return {k: (v[0] if k.endswith("/ref_images") else v) for k, v in out.items()}


def cases(g):
    """[(case, bits)] in a fixed order"""
    names = sorted({k.split("/")[0] for k in g}, key=lambda c: (int(c.split("x")[0]), int(c.split("x")[1].split("_")[0]), int(c.split("_")[1])))
    return [(c, int(c.split("_")[1])) for c in names]


def quantise(v, peak):
    """rint(clamp(v, 0, 1) * peak), half to even, in float64"""
    return np.rint(np.clip(np.asarray(v, np.float64), 0.0, 1.0) * peak)
