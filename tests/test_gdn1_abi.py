"""CPU: the C ABI of the GDN1 kernels (include/stem_gdn1.h: stem_gdn1_fwd, stem_gdn1_bwd_workspace_bytes, stem_gdn1_bwd; csrc/gdn1.hip).
Argument errors name their function and are reported before anything touches a device, and empty calls return 0 without a launch, so
all of this runs without one."""
import ctypes as C
import os
import re

import pytest

NEW = ("stem_gdn1_bwd", "stem_gdn1_bwd_workspace_bytes", "stem_gdn1_fwd")
NARGS = {"stem_gdn1_fwd": 11, "stem_gdn1_bwd_workspace_bytes": 2, "stem_gdn1_bwd": 17}
P = 4096                      # a 16-byte aligned "pointer": never dereferenced, every call below returns before a launch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "stem_gdn1.h")


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def _macro(name):
    return int(re.search(rf"^#define {name} (\d+)", open(HEADER).read(), flags=re.M).group(1))


def test_symbols_are_declared_bound_and_off_the_tape():
    """include/stem_gdn1.h is read and bound like stem_eb_filters.h; its entry points are additive (the ABI version stays 5) and outside
    the launch tape's table, which lists stem_hip.h's entry points"""
    from spatiotemporalentropymodel_amd import _abi
    lib = _lib()
    protos = _abi.prototypes(HEADER)
    assert lib.declared_hip_gdn1_symbols() == sorted(NEW) == sorted(protos)
    assert {n: len(a) for n, (_, a) in protos.items()} == NARGS
    assert protos["stem_gdn1_bwd_workspace_bytes"] == (C.c_size_t, [C.c_size_t, C.c_int])
    assert protos["stem_gdn1_fwd"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                                 C.c_float, C.c_void_p])
    assert protos["stem_gdn1_bwd"][0] is C.c_int and protos["stem_gdn1_bwd"][1][10:] == [C.c_size_t, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                                                                          C.c_size_t, C.c_void_p]
    others = (set(lib.declared_hip_symbols()) | set(lib.declared_hip_batch_symbols()) | set(lib.declared_hip_block_symbols()) |
              set(lib.declared_hip_hyperprior_symbols()) | set(lib.declared_hip_eb_filters_symbols()))
    assert not set(NEW) & others
    assert len(lib.declared_hip_symbols()) == 146                      # stem_hip.h, and with it the tape's table, is untouched
    raw = C.CDLL(lib.HIP_SO)
    h = lib.hip()
    assert h.stem_abi_version() == 5
    for name in NEW:
        fn = getattr(h, name)
        assert fn.restype is protos[name][0] and len(fn.argtypes) == NARGS[name], name
        assert h.stem_tape_entry_recordable(C.cast(getattr(raw, name), C.c_void_p)) == 0, name
    text = open(os.path.join(REPO, "spatiotemporalentropymodel_amd", "csrc", "tape_entries.inc")).read()
    assert not any(name in text for name in NEW)


def test_the_header_states_the_cap_and_the_chunk():
    lib = _lib()
    assert _macro("STEM_GDN1_MAX_C") >= 320 and _macro("STEM_GDN1_PIX_CHUNK") >= 32
    assert lib.header_macro("stem_gdn1.h", "STEM_GDN1_MAX_C") == _macro("STEM_GDN1_MAX_C")
    assert lib.header_macro("stem_gdn1.h", "STEM_GDN1_PIX_CHUNK") == _macro("STEM_GDN1_PIX_CHUNK")
    with pytest.raises(lib.StemLibraryError):
        lib.header_macro("stem_gdn1.h", "STEM_GDN1_NO_SUCH_MACRO")


def _fwd(h, **kw):
    a = dict(dict(x=P, ldx=8, beta=P, gamma=P, y=P, ldy=8, npix=5, C=8, inverse=0), **kw)
    return h.stem_gdn1_fwd(a["x"], a["ldx"], a["beta"], a["gamma"], a["y"], a["ldy"], a["npix"], a["C"], a["inverse"], 1e-6, None)


def _bwd(h, **kw):
    a = dict(dict(x=P, ldx=8, dy=P, lddy=8, beta=P, gamma=P, dx=P, lddx=8, dbeta=P, dgamma=P, npix=5, C=8, inverse=0, ws=P, short=0), **kw)
    need = h.stem_gdn1_bwd_workspace_bytes(max(a["npix"], 0), a["C"])
    return h.stem_gdn1_bwd(a["x"], a["ldx"], a["dy"], a["lddy"], a["beta"], a["gamma"], a["dx"], a["lddx"], a["dbeta"], a["dgamma"], a["npix"],
                           a["C"], a["inverse"], 1e-6, a["ws"], max(need - a["short"], 0), None)


def _cases():
    cap = _macro("STEM_GDN1_MAX_C")
    return {"stem_gdn1_fwd": (_fwd, (dict(x=None), dict(beta=None), dict(gamma=None), dict(y=None), dict(C=0), dict(C=-4), dict(C=cap + 1),
                                     dict(C=cap + 4, ldx=cap + 4, ldy=cap + 4), dict(ldx=7), dict(ldy=7), dict(C=3, ldy=2))),
            "stem_gdn1_bwd": (_bwd, (dict(x=None), dict(dy=None), dict(beta=None), dict(gamma=None), dict(C=0), dict(C=-1), dict(C=cap + 1),
                                     dict(dx=None, dbeta=None, dgamma=None), dict(dbeta=None), dict(dgamma=None), dict(short=1), dict(ws=None),
                                     dict(ws=P + 4), dict(ldx=7), dict(lddy=7), dict(lddx=7)))}


@pytest.mark.parametrize("name", ["stem_gdn1_fwd", "stem_gdn1_bwd"])
def test_argument_errors_name_the_function(name):
    h = _lib().hip()
    call, cases = _cases()[name]
    for bad in cases:
        assert call(h, **bad) == -1 and name.encode() in h.stem_last_error(), (name, bad, h.stem_last_error())
    assert call(h, **cases[-1]) == -1 and b"smaller than C" in h.stem_last_error()
    if name == "stem_gdn1_bwd":
        assert call(h, short=1) == -1 and b"workspace too small" in h.stem_last_error()
        assert call(h, dx=None, dbeta=None, dgamma=None) == -1 and b"all NULL" in h.stem_last_error()


@pytest.mark.parametrize("name", ["stem_gdn1_fwd", "stem_gdn1_bwd"])
def test_empty_calls_return_zero_without_a_launch(name):
    """npix == 0: 0, whatever else is passed (nothing is launched, so no device is needed)"""
    h = _lib().hip()
    call, _ = _cases()[name]
    assert call(h, npix=0) == 0
    assert call(h, npix=0, C=3) == 0
    assert call(h, npix=0, x=None, beta=None, gamma=None, C=10 ** 6) == 0


def test_workspace_size():
    h = _lib().hip()
    cap, chunk = _macro("STEM_GDN1_MAX_C"), _macro("STEM_GDN1_PIX_CHUNK")
    assert h.stem_gdn1_bwd_workspace_bytes(0, 8) == 0 and h.stem_gdn1_bwd_workspace_bytes(5, 0) == 0
    assert h.stem_gdn1_bwd_workspace_bytes(5, cap + 1) == 0
    for Cc in (1, 3, 36, cap):
        sizes = [h.stem_gdn1_bwd_workspace_bytes(n, Cc) for n in (1, 2, 63, 64, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 10 * chunk, 1 << 22)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] >= 4 * (Cc + Cc * Cc + Cc), (Cc, sizes)
        # one [npix][C] tensor and one [C][C] + [C] partial per chunk: nothing else of the activation's size
        n = 10 * chunk
        assert sizes[-2] <= 4 * (n * Cc + 4 + 10 * (Cc * Cc + Cc))
