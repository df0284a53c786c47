"""CPU: the C ABI of the per-frame passes of the pixel-domain sequence codec (include/stem_roiio.h: stem_rgb_window_recondition,
stem_roi_map_padded; csrc/roiio.hip, libstem_roiio.so).  Argument errors name their function and are reported before anything touches a
device, so all of this runs without one."""
import ctypes as C
import os
import subprocess

import pytest

NEW = ("stem_rgb_window_recondition", "stem_roi_map_padded", "stem_roiio_last_error")
NARGS = {"stem_rgb_window_recondition": 16, "stem_roi_map_padded": 12, "stem_roiio_last_error": 0}
P = 4096                      # a 16-byte aligned "pointer": never dereferenced, every call below returns before a launch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "stem_roiio.h")
OTHER_HEADERS = ("stem_hip.h", "stem_ar_batch.h", "stem_blocks.h", "stem_hyperprior.h", "stem_eb_filters.h", "stem_gdn1.h", "stem_validation.h",
                 "stem_frameio.h", "stem_rans.h", "stem_dp.h")


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def test_the_header_parses_and_is_bound_off_the_tape():
    """include/stem_roiio.h is read and bound like stem_frameio.h; its entry points are additive (the ABI version stays 5, stem_hip.h keeps
    its 146 entry points) and outside the launch tape's table"""
    from spatiotemporalentropymodel_amd import _abi
    lib = _lib()
    protos = _abi.prototypes(HEADER)
    assert lib.declared_roiio_symbols() == sorted(NEW) == sorted(protos)
    assert {n: len(a) for n, (_, a) in protos.items()} == NARGS
    v, i, z, f = C.c_void_p, C.c_int, C.c_size_t, C.c_float
    assert protos["stem_rgb_window_recondition"] == (i, [v, i, i, i, z, z, i, i, i, i, v, v, v, i, i, v])
    assert protos["stem_roi_map_padded"] == (i, [v, v, i, f, v, i, i, i, i, i, i, v])
    assert protos["stem_roiio_last_error"] == (C.c_char_p, [])
    assert lib.header_macro("stem_roiio.h", "STEM_ROI_MAX_BOXES") == 64
    others = set()
    for h in OTHER_HEADERS:
        others |= set(_abi.prototypes(os.path.join(REPO, "include", h)))
    assert not set(NEW) & others
    assert len(lib.declared_hip_symbols()) == 146                      # stem_hip.h, and with it the tape's table, is untouched
    assert lib.hip().stem_abi_version() == 5
    r = lib.roiio()
    for name in NEW:
        fn = getattr(r, name)
        assert fn.restype is protos[name][0] and len(fn.argtypes) == NARGS[name], name
    text = open(os.path.join(REPO, "spatiotemporalentropymodel_amd", "csrc", "tape_entries.inc")).read()
    assert not any(name in text for name in NEW)


def test_the_libraries_export_exactly_what_the_headers_declare():
    """libstem_roiio.so exports the header's three names and nothing else of the project's; the other two HIP libraries export none of them"""
    lib = _lib()

    def exported(so):
        out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    assert {n for n in exported(lib.ROIIO_SO) if n.startswith("stem_")} == set(NEW)
    assert not set(NEW) & exported(lib.HIP_SO)
    assert not set(NEW) & exported(lib.FRAMEIO_SO)


def _recondition(r, **kw):
    a = dict(dict(rgb=P, B=2, Hp=64, Wp=64, row=64, plane=64 * 64, top=29, left=27, H=6, W=10, y=P, u=P, v=P, sb=1, bits=8), **kw)
    return r.stem_rgb_window_recondition(a["rgb"], a["B"], a["Hp"], a["Wp"], a["row"], a["plane"], a["top"], a["left"], a["H"], a["W"], a["y"],
                                         a["u"], a["v"], a["sb"], a["bits"], None)


def _roi_map(r, **kw):
    a = dict(dict(boxes=P, values=P, n=3, bg=0.25, map=P, Hp=64, Wp=64, top=29, left=27, H=6, W=10), **kw)
    return r.stem_roi_map_padded(a["boxes"], a["values"], a["n"], a["bg"], a["map"], a["Hp"], a["Wp"], a["top"], a["left"], a["H"], a["W"], None)


RECONDITION_BAD = [dict(rgb=None), dict(y=None), dict(u=None), dict(v=None), dict(y=None, u=None), dict(u=None, v=None), dict(y=None, v=None),
                   dict(rgb=None, y=None, u=None, v=None), dict(B=0), dict(H=5), dict(W=9), dict(H=0), dict(W=0), dict(sb=3), dict(bits=9), dict(bits=10),
                   dict(top=-1), dict(left=-1), dict(top=59), dict(left=55), dict(Hp=4), dict(Wp=8), dict(Hp=0), dict(row=63),
                   dict(plane=64 * 64 - 1), dict(row=70, plane=64 * 70 - 7), dict(u=P + 1, sb=2, bits=10), dict(rgb=P + 2),
                   dict(y=None, u=None, v=None, H=5), dict(y=None, u=None, v=None, top=59), dict(y=None, u=None, v=None, row=63)]
ROI_MAP_BAD = [dict(map=None), dict(boxes=None), dict(values=None), dict(boxes=None, values=None), dict(n=-1), dict(n=65), dict(H=0), dict(W=0),
               dict(top=-1), dict(left=-1), dict(top=59), dict(left=55), dict(Hp=4), dict(Wp=8), dict(Hp=0), dict(Wp=0), dict(map=P + 2),
               dict(boxes=P + 1), dict(values=P + 2), dict(n=0, boxes=None, values=None, map=None)]


@pytest.mark.parametrize("kw", RECONDITION_BAD, ids=str)
def test_recondition_refuses_before_launch(kw):
    r = _lib().roiio()
    assert _recondition(r, **kw) == -1 and b"stem_rgb_window_recondition" in r.stem_roiio_last_error(), r.stem_roiio_last_error()


@pytest.mark.parametrize("kw", ROI_MAP_BAD, ids=str)
def test_roi_map_refuses_before_launch(kw):
    r = _lib().roiio()
    assert _roi_map(r, **kw) == -1 and b"stem_roi_map_padded" in r.stem_roiio_last_error(), r.stem_roiio_last_error()


def test_the_wrappers_refuse_host_tensors_and_bad_boxes():
    import torch
    from spatiotemporalentropymodel_amd import functional as F
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.rgb_window_recondition(torch.zeros(1, 3, 64, 64), (4, 4), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.rgb_window_recondition(torch.zeros(1, 3, 64, 64), (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.roi_map_padded([(0, 0, 2, 2, 0.5)], (4, 4), device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            F.roi_map_padded([(0, 0, 2, 2, 0.5)], (4, 4))
    good = [(0, 0, 2, 2, 0.5), (-5, 1, 9, 3, 1.0, 2)]
    assert F.roi_boxes_check(good, 0.25) == ([(0, 0, 2, 2, 0), (-5, 1, 9, 3, 2)], [0.5, 1.0], 0.25)
    assert F.roi_boxes_check([], 0) == ([], [], 0.0)
    bad = [[(2, 0, 2, 2, 0.5)], [(3, 0, 2, 2, 0.5)], [(0, 2, 2, 2, 0.5)], [(0, 3, 2, 2, 0.5)], [(0, 0, 2, 2, 1.5)], [(0, 0, 2, 2, -0.1)],
           [(0, 0, 2, 2, float("nan"))], [(0, 0, 2, 2, 0.5, -1)], [(0, 0, 2, 2, 0.5, 1.5)], [(0.5, 0, 2, 2, 0.5)], [(0, 0, 2, 2)],
           [(0, 0, 2, 2, 0.5, 1, 7)], [(0, 0, 2 ** 31, 2, 0.5)], [(0, 0, 2, 2, 0.5)] * 65]
    for boxes in bad:
        with pytest.raises(ValueError, match="roi_map_padded"):
            F.roi_boxes_check(boxes)
    for background in (-0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="background"):
            F.roi_boxes_check(good, background)
