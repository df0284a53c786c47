"""CPU: the C ABI of the conditioning-state hash (include/stem_statehash.h: stem_state_hash, stem_state_hash_workspace_bytes; csrc/statehash.hip,
libstem_statehash.so).  Argument errors name their function and are reported before anything touches a device, so all of this runs
without one."""
import ctypes as C
import os
import subprocess

import pytest

NEW = ("stem_state_hash", "stem_state_hash_workspace_bytes", "stem_statehash_last_error")
NARGS = {"stem_state_hash": 13, "stem_state_hash_workspace_bytes": 4, "stem_statehash_last_error": 0}
P = 4096                      # a 16-byte aligned "pointer": never dereferenced, every call below returns before a launch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "stem_statehash.h")
OTHER_HEADERS = ("stem_hip.h", "stem_ar_batch.h", "stem_blocks.h", "stem_hyperprior.h", "stem_eb_filters.h", "stem_gdn1.h", "stem_validation.h",
                 "stem_frameio.h", "stem_roiio.h", "stem_tail.h", "stem_rans.h", "stem_dp.h")


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def test_the_header_parses_and_is_bound_off_the_tape():
    """include/stem_statehash.h is read and bound like stem_roiio.h; its entry points are additive (the ABI version stays 5, stem_hip.h
    keeps its 146 entry points) and outside the launch tape's table"""
    from spatiotemporalentropymodel_amd import _abi
    lib = _lib()
    protos = _abi.prototypes(HEADER)
    assert lib.declared_statehash_symbols() == sorted(NEW) == sorted(protos)
    assert {n: len(a) for n, (_, a) in protos.items()} == NARGS
    v, i, z = C.c_void_p, C.c_int, C.c_size_t
    assert protos["stem_state_hash"] == (i, [v, i, i, i, i, z, z, z, z, v, v, z, v])
    assert protos["stem_state_hash_workspace_bytes"] == (z, [i, i, i, i])
    assert protos["stem_statehash_last_error"] == (C.c_char_p, [])
    chunk = lib.header_macro("stem_statehash.h", "STEM_STATE_HASH_CHUNK")
    assert chunk >= 64 and chunk % 4 == 0
    others = set()
    for h in OTHER_HEADERS:
        others |= set(_abi.prototypes(os.path.join(REPO, "include", h)))
    assert not set(NEW) & others
    assert len(lib.declared_hip_symbols()) == 146                      # stem_hip.h, and with it the tape's table, is untouched
    assert lib.hip().stem_abi_version() == 5
    s = lib.statehash()
    for name in NEW:
        fn = getattr(s, name)
        assert fn.restype is protos[name][0] and len(fn.argtypes) == NARGS[name], name
    for inc in ("tape_entries.inc", "tape_entries_tail.inc"):
        text = open(os.path.join(REPO, "spatiotemporalentropymodel_amd", "csrc", inc)).read()
        assert not any(name in text for name in NEW)


def test_the_libraries_export_exactly_what_the_headers_declare():
    """libstem_statehash.so exports the header's three names and nothing else of the project's; the three older HIP libraries export
    none of them and still exactly their own headers' names"""
    lib = _lib()

    def exported(so):
        out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    assert {n for n in exported(lib.STATEHASH_SO) if n.startswith("stem_")} == set(NEW)
    for so in (lib.HIP_SO, lib.FRAMEIO_SO, lib.ROIIO_SO):
        assert not set(NEW) & exported(so), so
    assert {n for n in exported(lib.FRAMEIO_SO) if n.startswith("stem_")} == set(lib.declared_frameio_symbols())
    assert {n for n in exported(lib.ROIIO_SO) if n.startswith("stem_")} == set(lib.declared_roiio_symbols())


def test_workspace_bytes():
    lib = _lib()
    s = lib.statehash()
    chunk = lib.header_macro("stem_statehash.h", "STEM_STATE_HASH_CHUNK")
    assert s.stem_state_hash_workspace_bytes(1, 1, 1, chunk) == 0
    assert s.stem_state_hash_workspace_bytes(3, 1, 1, chunk) == 0
    assert s.stem_state_hash_workspace_bytes(1, 1, 1, chunk + 1) == 16
    assert s.stem_state_hash_workspace_bytes(3, 2, chunk, 5) == 3 * 10 * 8
    assert s.stem_state_hash_workspace_bytes(0, 1, 1, 1) == 0
    assert s.stem_state_hash_workspace_bytes(1, 1 << 20, 1 << 12, 2) == 0          # refused by the call: nothing to size


def _hash(s, **kw):
    """a dense planar [2, 3, 40, 50] call (two chunks an image) unless told otherwise"""
    a = dict(dict(x=P, B=2, C=3, H=40, W=50, sb=6000, sc=2000, sh=50, sw=1, out=P, ws=P, wsb=1 << 20), **kw)
    return s.stem_state_hash(a["x"], a["B"], a["C"], a["H"], a["W"], a["sb"], a["sc"], a["sh"], a["sw"], a["out"], a["ws"], a["wsb"], None)


CL = dict(sb=6000, sc=1, sh=150, sw=3)                                    # the same tensor channels-last
BAD = [dict(x=None), dict(out=None), dict(ws=None), dict(x=None, out=None, ws=None),                       # null pointers
       dict(wsb=0), dict(wsb=2 * 2 * 8 - 1),                                                               # a workspace that is too small
       dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(B=-1), dict(W=-5), dict(B=65536),                  # extents
       dict(B=1, C=1 << 16, H=1 << 16, W=2, sc=1 << 17, sh=2), dict(B=1, C=1 << 30, H=1 << 30, W=1 << 30),  # C * H * W > 2^32
       dict(sw=2), dict(sh=49), dict(sc=1999), dict(sb=5999), dict(sw=0), dict(sh=0), dict(sc=0), dict(sb=0),  # planar strides
       dict(CL, sw=2), dict(CL, sh=149), dict(CL, sc=2), dict(CL, sb=5999), dict(CL, sw=0),                   # channels-last strides
       dict(sb=2000 * 50, sc=50, sh=1, sw=2000 * 50 * 3),                                                  # a permuted view
       dict(sc=1 << 40), dict(sb=1 << 41), dict(sh=1 << 39, sc=1 << 39),                                   # absurd pitches
       dict(x=P + 2), dict(out=P + 4), dict(ws=P + 4)]                                                     # misaligned pointers


@pytest.mark.parametrize("kw", BAD, ids=str)
def test_state_hash_refuses_before_launch(kw):
    s = _lib().statehash()
    assert _hash(s, **kw) < 0 and b"stem_state_hash" in s.stem_statehash_last_error(), s.stem_statehash_last_error()


def test_the_wrapper_refuses_host_tensors_other_types_and_other_layouts():
    import torch
    from spatiotemporalentropymodel_amd import functional as F
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.state_hash(torch.zeros(1, 3, 4, 4))
    x = torch.zeros(2, 6, 5, 7)
    assert F.state_hash_strides(x.shape, x.stride()) == (210, 35, 7, 1)
    cl = x.contiguous(memory_format=torch.channels_last)
    assert F.state_hash_strides(cl.shape, cl.stride()) == (210, 1, 42, 6)
    big = torch.zeros(2, 6, 9, 10)[:, :, 2:7, 1:8]
    assert F.state_hash_strides(big.shape, big.stride()) == (540, 90, 10, 1)
    one = torch.zeros(1, 1, 5, 7).contiguous(memory_format=torch.channels_last)         # extents of 1 carry no stride of their own
    assert F.state_hash_strides(one.shape, one.stride())[1:] in ((35, 7, 1), (1, 7, 1))
    for bad in (x.permute(0, 1, 3, 2), x.permute(1, 0, 2, 3), x[:, :, :, ::2], cl[:, ::2], x.as_strided((2, 6, 5, 7), (0, 35, 7, 1))):
        with pytest.raises(ValueError, match="state_hash"):
            F.state_hash_strides(bad.shape, bad.stride())
    with pytest.raises(ValueError, match="state_hash"):
        F.state_hash_strides((0, 3, 4, 4), (48, 16, 4, 1))
    assert F.state_hash_ints(torch.tensor([-1, 0, 1 - 2 ** 63], dtype=torch.int64)) == [2 ** 64 - 1, 0, 2 ** 63 + 1]
