"""ctypes loader for the C-ABI libraries (include/stem_hip.h + include/stem_ar_batch.h + include/stem_blocks.h +
include/stem_hyperprior.h + include/stem_eb_filters.h + include/stem_gdn1.h + include/stem_validation.h, include/stem_tail.h, include/stem_frameio.h, include/stem_roiio.h, include/stem_statehash.h,
include/stem_rans.h, include/stem_dp.h).

The headers are the single statement of the ABI: every prototype and descriptor structure below is read from them (_abi.py).

The HIP library is the product compute path: there is NO CPU or PyTorch fallback.  If
libstem_hip.so is missing every device op raises (loudly), it never silently degrades.
"""
from __future__ import annotations

import ctypes as C
import os
import re

from . import _abi

_PKG = os.path.dirname(os.path.abspath(__file__))
# STEM_HIP_LIBRARY names another build of the same ABI (`make variant` -> libstem_hip_<tag>.so, tools/debug/ab_lib.sh)
HIP_SO = os.environ.get("STEM_HIP_LIBRARY") or os.path.join(_PKG, "libstem_hip.so")
# STEM_RANS_LIBRARY names another build of the host codec (`make sanitize` -> libstem_rans_asan.so, the sanitizer test)
RANS_SO = os.environ.get("STEM_RANS_LIBRARY") or os.path.join(_PKG, "libstem_rans.so")

# the frame ingest / emit kernels of the sequence codec (include/stem_frameio.h): a library of their own
FRAMEIO_SO = os.path.join(_PKG, "libstem_frameio.so")
# the optimiser pass over a table of chunk ranges (include/stem_tail.h): a library of its own too
TAIL_SO = os.path.join(_PKG, "libstem_tail.so")
# the per-frame passes of the pixel-domain sequence codec (include/stem_roiio.h): a library of their own as well
ROIIO_SO = os.path.join(_PKG, "libstem_roiio.so")
# the conditioning-state hash of the sequence codecs (include/stem_statehash.h): a library of its own as well
STATEHASH_SO = os.path.join(_PKG, "libstem_statehash.so")
DP_SO = os.environ.get("STEM_DP_LIBRARY") or os.path.join(_PKG, "libstem_dp.so")
_hip = None
_rans = None
_dp = None
_frameio = None
_tail = None
_roiio = None
_statehash = None


class StemLibraryError(RuntimeError):
    pass


def _header(name):
    path = os.path.join(_PKG, "..", "include", name)
    if not os.path.exists(path):
        raise StemLibraryError(f"{path} is missing: the ctypes prototypes and structures are read from the C headers")
    return path


def _tables(header):
    """include/<header> as ctypes sees it: name -> (restype, argtypes), name -> argtypes, name -> restype where it is not int"""
    protos = _abi.prototypes(_header(header))
    return protos, {n: args for n, (_, args) in protos.items()}, {n: res for n, (res, _) in protos.items() if res is not C.c_int}


# tape.py classifies the argument slots of a recorded call by _HIP_SIG (with stem_tail.h's: _TAPE_SIG below) and leaves the entries of _RESTYPE out of a schedule
_HIP_PROTO, _HIP_SIG, _RESTYPE = _tables("stem_hip.h")
# libstem_hip.so's batched coding entry points (not launch-tape entries: tape.py does not see them)
_HIP_BATCH_PROTO, _HIP_BATCH_SIG, _ = _tables("stem_ar_batch.h")
# libstem_hip.so's block kernels of the cheng2020 models (csrc/resblock.hip; not launch-tape entries either)
_HIP_BLOCKS_PROTO, _HIP_BLOCKS_SIG, _ = _tables("stem_blocks.h")
# libstem_hip.so's zero-mean likelihood kernels of the bmshj2018 models (csrc/hyperprior.hip; not launch-tape entries either)
_HIP_HYPERPRIOR_PROTO, _HIP_HYPERPRIOR_SIG, _ = _tables("stem_hyperprior.h")
# libstem_hip.so's EntropyBottleneck kernels for any `filters` tuple (csrc/eb_filters.hip; not launch-tape entries either)
_HIP_EBF_PROTO, _HIP_EBF_SIG, _ = _tables("stem_eb_filters.h")
# libstem_hip.so's GDN1 kernels (csrc/gdn1.hip; not launch-tape entries either)
_HIP_GDN1_PROTO, _HIP_GDN1_SIG, _ = _tables("stem_gdn1.h")
# libstem_hip.so's eval-mode rate kernels and running loss sum of the validation pass (csrc/entropy.hip; not launch-tape entries either)
_HIP_VALIDATION_PROTO, _HIP_VALIDATION_SIG, _ = _tables("stem_validation.h")
# libstem_tail.so's optimiser pass over a table of chunk ranges (csrc/tail.hip): a launch-tape entry like stem_hip.h's, checked and
# listed by its own library (csrc/tape_entries_tail.inc, stem_tail_entry_recordable)
_TAIL_PROTO, _TAIL_SIG, _ = _tables("stem_tail.h")
#: every entry point a launch tape may hold: what tape.py classifies the argument slots of a recorded call by
_TAPE_SIG = {**_HIP_SIG, **{n: a for n, a in _TAIL_SIG.items() if not n.startswith("stem_tail_")}}
# libstem_frameio.so's padded-frame ingest and window emit kernels (csrc/frameio.hip; not launch-tape entries either)
_FRAMEIO_PROTO, _FRAMEIO_SIG, _ = _tables("stem_frameio.h")
# libstem_roiio.so's recondition and ROI rasteriser kernels (csrc/roiio.hip; not launch-tape entries either)
_ROIIO_PROTO, _ROIIO_SIG, _ = _tables("stem_roiio.h")
# libstem_statehash.so's per-image hash of a conditioning state (csrc/statehash.hip; not a launch-tape entry either)
_STATEHASH_PROTO, _STATEHASH_SIG, _ = _tables("stem_statehash.h")
_RANS_PROTO, _RANS_SIG, _RANS_RESTYPE = _tables("stem_rans.h")
_DP_PROTO, _DP_SIG, _ = _tables("stem_dp.h")
_STRUCTS = _abi.structs(_header("stem_hip.h"))


class PackDesc(C.Structure):
    _fields_ = _STRUCTS["stem_pack_desc"]


class F16PackDesc(C.Structure):
    _fields_ = _STRUCTS["stem_f16x2_pack_desc"]


class F16PairDesc(C.Structure):
    _fields_ = _STRUCTS["stem_f16x2_pair_desc"]


class UnpackDesc(C.Structure):
    _fields_ = _STRUCTS["stem_unpack_desc"]


class BiasFinalDesc(C.Structure):
    _fields_ = _STRUCTS["stem_bias_final_desc"]


class WaveSeg(C.Structure):
    _fields_ = _STRUCTS["stem_wave_seg"]


def _bind(lib, protos):
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export a declared symbol
        fn.argtypes = argtypes
        fn.restype = restype
    return lib


def hip():
    """libstem_hip.so, or raise: the product path has no fallback."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_SO):
            raise StemLibraryError(
                f"{HIP_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the STEM kernels.")
        lib = C.CDLL(HIP_SO)
        for protos in (_HIP_PROTO, _HIP_BATCH_PROTO, _HIP_BLOCKS_PROTO, _HIP_HYPERPRIOR_PROTO, _HIP_EBF_PROTO, _HIP_GDN1_PROTO,
                       _HIP_VALIDATION_PROTO):
            _bind(lib, protos)
        _hip = lib
    return _hip


def frameio():
    """libstem_frameio.so (include/stem_frameio.h), or raise: like libstem_hip.so it has no fallback"""
    global _frameio
    if _frameio is None:
        if not os.path.exists(FRAMEIO_SO):
            raise StemLibraryError(f"{FRAMEIO_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                   "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the frame kernels.")
        _frameio = _bind(C.CDLL(FRAMEIO_SO), _FRAMEIO_PROTO)
    return _frameio


def tail():
    """libstem_tail.so (include/stem_tail.h), or raise: like libstem_hip.so it has no fallback"""
    global _tail
    if _tail is None:
        if not os.path.exists(TAIL_SO):
            raise StemLibraryError(f"{TAIL_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                   "(hipcc --offload-arch=gfx950).  There is no fallback for the ordered optimiser tail's kernel.")
        _tail = _bind(C.CDLL(TAIL_SO), _TAIL_PROTO)
    return _tail


def check_tail(rc: int):
    if rc != 0:
        raise RuntimeError((tail().stem_tail_last_error() or b"").decode() or f"libstem_tail error {rc}")


def check_frameio(rc: int):
    if rc != 0:
        raise RuntimeError((frameio().stem_frameio_last_error() or b"").decode() or f"libstem_frameio error {rc}")


def roiio():
    """libstem_roiio.so (include/stem_roiio.h), or raise: like libstem_hip.so it has no fallback"""
    global _roiio
    if _roiio is None:
        if not os.path.exists(ROIIO_SO):
            raise StemLibraryError(f"{ROIIO_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                   "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the frame kernels.")
        _roiio = _bind(C.CDLL(ROIIO_SO), _ROIIO_PROTO)
    return _roiio


def check_roiio(rc: int):
    if rc != 0:
        raise RuntimeError((roiio().stem_roiio_last_error() or b"").decode() or f"libstem_roiio error {rc}")


def statehash():
    """libstem_statehash.so (include/stem_statehash.h), or raise: like libstem_hip.so it has no fallback"""
    global _statehash
    if _statehash is None:
        if not os.path.exists(STATEHASH_SO):
            raise StemLibraryError(f"{STATEHASH_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                   "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the state hash.")
        _statehash = _bind(C.CDLL(STATEHASH_SO), _STATEHASH_PROTO)
    return _statehash


def check_statehash(rc: int):
    if rc != 0:
        raise RuntimeError((statehash().stem_statehash_last_error() or b"").decode() or f"libstem_statehash error {rc}")


def rans():
    global _rans
    if _rans is None:
        if not os.path.exists(RANS_SO):
            raise StemLibraryError(f"{RANS_SO} is missing: run `make -C {os.path.join(_PKG, 'csrc')}`")
        _rans = _bind(C.CDLL(RANS_SO), _RANS_PROTO)
    return _rans


def check(rc: int):
    if rc != 0:
        raise RuntimeError((hip().stem_last_error() or b"").decode() or f"libstem_hip error {rc}")


def declared_hip_symbols():
    return sorted(_HIP_SIG)


def declared_hip_batch_symbols():
    return sorted(_HIP_BATCH_SIG)


def declared_hip_block_symbols():
    return sorted(_HIP_BLOCKS_SIG)


def declared_hip_hyperprior_symbols():
    return sorted(_HIP_HYPERPRIOR_SIG)


def declared_hip_eb_filters_symbols():
    return sorted(_HIP_EBF_SIG)


def declared_hip_gdn1_symbols():
    return sorted(_HIP_GDN1_SIG)


def declared_hip_validation_symbols():
    return sorted(_HIP_VALIDATION_SIG)


def declared_tail_symbols():
    return sorted(_TAIL_SIG)


def declared_frameio_symbols():
    return sorted(_FRAMEIO_SIG)


def declared_roiio_symbols():
    return sorted(_ROIIO_SIG)


def declared_statehash_symbols():
    return sorted(_STATEHASH_SIG)


def header_macro(header, name):
    """integer value of `#define <name> <integer>` in include/<header> (the caps and chunk sizes the headers state)"""
    m = re.search(rf"^[ \t]*#[ \t]*define[ \t]+{name}[ \t]+(\d+)\b", open(_header(header)).read(), flags=re.M)
    if not m:
        raise StemLibraryError(f"include/{header} does not define {name} as an integer")
    return int(m.group(1))


def dp():
    """libstem_dp.so (include/stem_dp.h): the native RCCL issue path of a data-parallel rank; links librccl"""
    global _dp
    if _dp is None:
        if not os.path.exists(DP_SO):
            raise StemLibraryError(f"{DP_SO} is missing: run `make -C {os.path.join(_PKG, 'csrc')}`")
        _dp = _bind(C.CDLL(DP_SO), _DP_PROTO)
    return _dp


def declared_dp_symbols():
    return sorted(_DP_SIG)


def declared_rans_symbols():
    return sorted(_RANS_SIG)
