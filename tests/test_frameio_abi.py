"""CPU: the C ABI of the frame ingest / emit kernels (include/stem_frameio.h: stem_yuv420_to_rgb_padded, stem_rgb_window_to_yuv420;
csrc/frameio.hip, libstem_frameio.so).  Argument errors name their function and are reported before anything touches a device, so all
of this runs without one."""
import ctypes as C
import os
import subprocess

import pytest

NEW = ("stem_frameio_last_error", "stem_rgb_window_to_yuv420", "stem_yuv420_to_rgb_padded")
NARGS = {"stem_yuv420_to_rgb_padded": 16, "stem_rgb_window_to_yuv420": 16, "stem_frameio_last_error": 0}
P = 4096                      # a 16-byte aligned "pointer": never dereferenced, every call below returns before a launch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "stem_frameio.h")
OTHER_HEADERS = ("stem_hip.h", "stem_ar_batch.h", "stem_blocks.h", "stem_hyperprior.h", "stem_eb_filters.h", "stem_gdn1.h", "stem_validation.h",
                 "stem_rans.h", "stem_dp.h")


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def test_the_header_parses_and_is_bound_off_the_tape():
    """include/stem_frameio.h is read and bound like stem_validation.h; its entry points are additive (the ABI version stays 5, stem_hip.h
    keeps its 146 entry points) and outside the launch tape's table"""
    from spatiotemporalentropymodel_amd import _abi
    lib = _lib()
    protos = _abi.prototypes(HEADER)
    assert lib.declared_frameio_symbols() == sorted(NEW) == sorted(protos)
    assert {n: len(a) for n, (_, a) in protos.items()} == NARGS
    v, i, z = C.c_void_p, C.c_int, C.c_size_t
    assert protos["stem_yuv420_to_rgb_padded"] == (i, [v, v, v, i, i, i, i, i, i, i, v, i, i, i, i, v])
    assert protos["stem_rgb_window_to_yuv420"] == (i, [v, i, i, i, z, z, i, i, i, i, v, v, v, i, i, v])
    assert protos["stem_frameio_last_error"] == (C.c_char_p, [])
    others = set()
    for h in OTHER_HEADERS:
        others |= set(_abi.prototypes(os.path.join(REPO, "include", h)))
    assert not set(NEW) & others
    assert len(lib.declared_hip_symbols()) == 146                      # stem_hip.h, and with it the tape's table, is untouched
    assert lib.hip().stem_abi_version() == 5
    f = lib.frameio()
    for name in NEW:
        fn = getattr(f, name)
        assert fn.restype is protos[name][0] and len(fn.argtypes) == NARGS[name], name
    text = open(os.path.join(REPO, "spatiotemporalentropymodel_amd", "csrc", "tape_entries.inc")).read()
    assert not any(name in text for name in NEW)


def test_the_libraries_export_exactly_what_the_headers_declare():
    """libstem_frameio.so exports the header's three names and nothing else of the project's; libstem_hip.so exports none of them"""
    lib = _lib()

    def exported(so):
        out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    assert {n for n in exported(lib.FRAMEIO_SO) if n.startswith("stem_")} == set(NEW)
    assert not set(NEW) & exported(lib.HIP_SO)


def _ingest(f, **kw):
    a = dict(dict(y=P, u=P, v=P, B=2, H=6, W=10, sb=1, bits=8, up=0, rgb=P, Hp=64, Wp=64, top=29, left=27), **kw)
    return f.stem_yuv420_to_rgb_padded(a["y"], a["u"], a["v"], a["B"], a["H"], a["W"], a["sb"], a["bits"], a["up"], 1, a["rgb"], a["Hp"], a["Wp"],
                                       a["top"], a["left"], None)


def _emit(f, **kw):
    a = dict(dict(rgb=P, B=2, Hp=64, Wp=64, row=64, plane=64 * 64, top=29, left=27, H=6, W=10, y=P, u=P, v=P, sb=1, bits=8), **kw)
    return f.stem_rgb_window_to_yuv420(a["rgb"], a["B"], a["Hp"], a["Wp"], a["row"], a["plane"], a["top"], a["left"], a["H"], a["W"], a["y"],
                                       a["u"], a["v"], a["sb"], a["bits"], None)


INGEST_BAD = [dict(y=None), dict(u=None), dict(v=None), dict(rgb=None), dict(B=0), dict(H=5), dict(W=9), dict(H=0), dict(sb=3), dict(bits=9),
              dict(bits=10), dict(up=2), dict(top=-1), dict(left=-1), dict(top=59), dict(left=55), dict(Hp=4), dict(Wp=8), dict(Hp=0), dict(y=P + 1, sb=2, bits=10),
              dict(rgb=P + 2)]
EMIT_BAD = [dict(rgb=None), dict(y=None), dict(u=None), dict(v=None), dict(B=0), dict(H=5), dict(W=9), dict(H=0), dict(sb=3), dict(bits=9),
            dict(bits=10), dict(top=-1), dict(left=-1), dict(top=59), dict(left=55), dict(Hp=4), dict(Wp=8), dict(row=63), dict(plane=64 * 64 - 1),
            dict(row=70, plane=64 * 70 - 7), dict(u=P + 1, sb=2, bits=10), dict(rgb=P + 2)]


@pytest.mark.parametrize("kw", INGEST_BAD, ids=str)
def test_ingest_refuses_before_launch(kw):
    f = _lib().frameio()
    assert _ingest(f, **kw) == -1 and b"stem_yuv420_to_rgb_padded" in f.stem_frameio_last_error(), f.stem_frameio_last_error()


@pytest.mark.parametrize("kw", EMIT_BAD, ids=str)
def test_emit_refuses_before_launch(kw):
    f = _lib().frameio()
    assert _emit(f, **kw) == -1 and b"stem_rgb_window_to_yuv420" in f.stem_frameio_last_error(), f.stem_frameio_last_error()


def test_the_wrappers_refuse_host_tensors_and_bad_geometry():
    import torch
    from spatiotemporalentropymodel_amd import functional as F
    assert F.pad_geometry(1080, 1920) == (1088, 1920, 4, 0) and F.pad_geometry(122, 126) == (128, 128, 3, 1) and F.pad_geometry(64, 64) == (64, 64, 0, 0)
    y, c = torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 2, 2, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.yuv420_to_rgb_padded(y, c, c, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.rgb_window_to_yuv420(torch.zeros(1, 3, 64, 64), (4, 4), 8)
