"""CPU: the C ABI of the one-shot coding kernels (include/stem_ar_batch.h: stem_symbols_pack, stem_symbols_unpack).  They are
declared in that header alone, exported, bound with the header's argument list, and refuse bad arguments before anything touches a
device, so all of this runs without one."""
import ctypes as C
import glob
import os
import re

from conftest import REPO

NAMES = ("stem_symbols_pack", "stem_symbols_unpack")
PACK_ARGS = ("y", "ldy", "means", "ldm", "chan_means", "scales", "lds", "table", "T", "scale_bound", "sym", "idx", "B", "H", "W", "C", "stream")
UNPACK_ARGS = ("sym", "means", "ldm", "chan_means", "y_hat", "ldo", "B", "H", "W", "C", "stream")


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def test_declared_in_the_batch_header_only():
    lib = _lib()
    assert set(NAMES) <= set(lib.declared_hip_batch_symbols())
    assert not set(NAMES) & set(lib.declared_hip_symbols())          # not launch-tape entries: tape.py does not see them
    for path in glob.glob(os.path.join(REPO, "include", "*.h")):
        text = open(path).read()
        for name in NAMES:
            assert (re.search(rf"\b{name}\s*\(", text) is not None) == path.endswith("stem_ar_batch.h"), (path, name)
    inc = open(os.path.join(REPO, "spatiotemporalentropymodel_amd", "csrc", "tape_entries.inc")).read()
    assert not any(name in inc for name in NAMES)
    assert lib.hip().stem_abi_version() == 5


def test_exported_and_bound_with_the_headers_argument_list():
    lib = _lib()
    raw = C.CDLL(lib.HIP_SO)
    for name in NAMES:
        assert getattr(raw, name) is not None
    h = lib.hip()
    header = open(os.path.join(REPO, "include", "stem_ar_batch.h")).read()
    p, i, f = C.c_void_p, C.c_int, C.c_float
    want = {"stem_symbols_pack": (PACK_ARGS, [p, i, p, i, p, p, i, p, i, f, p, p, i, i, i, i, p]),
            "stem_symbols_unpack": (UNPACK_ARGS, [p, p, i, p, p, i, i, i, i, i, p])}
    for name, (args, types) in want.items():
        fn = getattr(h, name)
        assert fn.restype is C.c_int
        assert len(fn.argtypes) == len(types)
        for k, (got, exp) in enumerate(zip(fn.argtypes, types)):
            if exp is p:                                               # a typed or an untyped pointer
                assert got is C.c_void_p or issubclass(got, C._Pointer), (name, args[k], got)
            else:
                assert got is exp, (name, args[k], got)
        decl = re.search(rf"int {name}\s*\(([^;]*)\);", header).group(1)
        names = [re.sub(r"[\s*]+", " ", a).strip().split(" ")[-1] for a in decl.split(",")]
        assert tuple(names) == args, (name, names)


def test_pack_refusals_name_the_function():
    h = _lib().hip()
    q = 4096                                           # never dereferenced: every call below fails its argument checks first
    ok = dict(y=q, ldy=8, means=q, ldm=8, chan_means=None, scales=q, lds=8, table=q, T=64, scale_bound=0.11, sym=q, idx=q, B=1, H=3, W=5, C=8)

    def call(**kw):
        a = dict(ok, **kw)
        rc = h.stem_symbols_pack(*[a[n] for n in PACK_ARGS[:-1]], None)
        return rc, h.stem_last_error()

    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(B=-3),                     # non-positive sizes
                dict(ldy=7), dict(ldm=7), dict(lds=7), dict(ldy=0),                          # a pitch below C
                dict(y=None, sym=None, means=None, idx=None, scales=None),                   # nothing to write
                dict(y=None, means=None), dict(sym=None),                                    # y and sym go together
                dict(chan_means=q),                                                          # both kinds of means
                dict(y=None, sym=None),                                                      # means without y
                dict(y=None, sym=None, means=None, chan_means=q),
                dict(idx=None),                                                              # scales without idx
                dict(table=None), dict(T=0), dict(T=-1)):                                    # scales without a table
        rc, msg = call(**bad)
        assert rc != 0 and b"stem_symbols_pack" in msg, (bad, rc, msg)
    assert b"at most one" in call(chan_means=q)[1] and b"ldm" in call(ldm=7)[1] and b"positive" in call(H=0)[1]


def test_unpack_refusals_name_the_function():
    h = _lib().hip()
    q = 4096
    ok = dict(sym=q, means=q, ldm=8, chan_means=None, y_hat=q, ldo=16, B=2, H=3, W=5, C=8)

    def call(**kw):
        a = dict(ok, **kw)
        rc = h.stem_symbols_unpack(*[a[n] for n in UNPACK_ARGS[:-1]], None)
        return rc, h.stem_last_error()

    for bad in (dict(sym=None), dict(y_hat=None), dict(chan_means=q), dict(ldm=7), dict(ldo=7), dict(ldo=0),
                dict(B=0), dict(H=0), dict(W=0), dict(C=-8)):
        rc, msg = call(**bad)
        assert rc != 0 and b"stem_symbols_unpack" in msg, (bad, rc, msg)
    assert b"at most one" in call(chan_means=q)[1] and b"ldo" in call(ldo=7)[1]


def test_functional_has_no_cpu_route():
    import pytest
    import torch
    from spatiotemporalentropymodel_amd import functional as F
    y = torch.zeros(1, 4, 2, 2).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    with pytest.raises(RuntimeError):
        F.symbols_pack(y)
    with pytest.raises(RuntimeError):
        F.symbols_unpack(torch.zeros(1, 4, 2, 2, dtype=torch.int32))
