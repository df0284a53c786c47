"""CPU: the C ABI of the block kernels (include/stem_blocks.h: stem_pixel_shuffle_fwd / _bwd, stem_add_act_fwd / _bwd, stem_gate_fwd /
_bwd; csrc/resblock.hip).  Argument errors name their function and are reported before anything touches a device, so all of this
runs without one."""
import ctypes as C

import pytest

NEW = ("stem_pixel_shuffle_fwd", "stem_pixel_shuffle_bwd", "stem_add_act_fwd", "stem_add_act_bwd", "stem_gate_fwd", "stem_gate_bwd")
P = 4096                      # a 16-byte aligned "pointer": never dereferenced, every call below fails its argument checks first


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def test_symbols_are_declared_and_exported():
    """include/stem_blocks.h is read and bound like the other headers of libstem_hip.so; its entry points are additive (the ABI version
    stays 5) and, like stem_ar_batch.h's, outside the launch tape's table, which lists stem_hip.h's entry points"""
    import os
    from spatiotemporalentropymodel_amd import _abi
    lib = _lib()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert lib.declared_hip_block_symbols() == sorted(NEW) == sorted(_abi.prototypes(os.path.join(repo, "include", "stem_blocks.h")))
    assert not set(NEW) & set(lib.declared_hip_symbols()) and not set(NEW) & set(lib.declared_hip_batch_symbols())
    raw = C.CDLL(lib.HIP_SO)
    h = lib.hip()
    assert h.stem_abi_version() == 5
    for name in NEW:
        fn = getattr(h, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(lib._HIP_BLOCKS_SIG[name]), name
        assert h.stem_tape_entry_recordable(C.cast(getattr(raw, name), C.c_void_p)) == 0, name
    text = open(os.path.join(repo, "spatiotemporalentropymodel_amd", "csrc", "tape_entries.inc")).read()
    assert not any(name in text for name in NEW)


def _shuffle_fwd(h, **kw):
    a = dict(dict(inp=P, ldi=32, addend=P, lda=8, out=P, ldo=8, B=1, H=2, W=3, C=8, r=2, slope=0.01), **kw)
    rc = h.stem_pixel_shuffle_fwd(a["inp"], a["ldi"], a["addend"], a["lda"], a["out"], a["ldo"], a["B"], a["H"], a["W"], a["C"], a["r"],
                                  a["slope"], None)
    return rc, h.stem_last_error()


def _shuffle_bwd(h, **kw):
    a = dict(dict(inp=P, ldi=32, dout=P, ldo=8, din=P, ldd=32, B=1, H=2, W=3, C=8, r=2, slope=0.01), **kw)
    rc = h.stem_pixel_shuffle_bwd(a["inp"], a["ldi"], a["dout"], a["ldo"], a["din"], a["ldd"], a["B"], a["H"], a["W"], a["C"], a["r"],
                                  a["slope"], None)
    return rc, h.stem_last_error()


def test_pixel_shuffle_argument_errors():
    h = _lib().hip()
    for call, name, cases in (
            (_shuffle_fwd, b"stem_pixel_shuffle_fwd",
             (dict(inp=None), dict(out=None), dict(r=0), dict(r=-1), dict(C=0), dict(C=-4), dict(ldi=31), dict(ldo=7), dict(lda=4),
              dict(ldi=34), dict(ldo=10), dict(lda=9), dict(inp=P + 4), dict(out=P + 8), dict(addend=P + 4), dict(B=-1),
              dict(C=3, ldi=11), dict(C=3, ldi=12, ldo=2), dict(C=1 << 20, r=1 << 10))),
            (_shuffle_bwd, b"stem_pixel_shuffle_bwd",
             (dict(dout=None), dict(din=None), dict(inp=None), dict(r=0), dict(C=0), dict(ldi=31), dict(ldo=7), dict(ldd=31), dict(ldi=34),
              dict(ldo=10), dict(ldd=33), dict(dout=P + 4), dict(din=P + 12), dict(inp=P + 4), dict(H=-1)))):
        for bad in cases:
            rc, msg = call(h, **bad)
            assert rc != 0 and name in msg, (name, bad, rc, msg)
    assert b"multiple of 4" in _shuffle_fwd(h, ldi=34)[1] and b"16-byte path" in _shuffle_fwd(h, ldo=10)[1]
    assert b"smaller than" in _shuffle_fwd(h, ldi=31)[1]
    assert b"r = 0" in _shuffle_fwd(h, r=0)[1] and b"C = 0" in _shuffle_bwd(h, C=0)[1]
    # what is NOT an error: no addend; C % 4 != 0 with any pitch >= C and any alignment; no `in` where there is no activation.
    # (empty tensors: nothing is launched, so these return 0 without a device)
    for ok in (dict(addend=None, B=0), dict(C=3, ldi=13, ldo=5, lda=3, inp=P + 4, out=P + 8, B=0), dict(H=0), dict(W=0)):
        rc, msg = _shuffle_fwd(h, **ok)
        assert rc == 0, (ok, msg)
    assert _shuffle_bwd(h, inp=None, slope=1.0, B=0)[0] == 0


def _elementwise_calls(h):
    def add_act_fwd(**kw):
        a = dict(dict(a=P, lda=8, b=P, ldb=8, out=P, ldo=8, npix=5, C=8, slope=0.0), **kw)
        return h.stem_add_act_fwd(a["a"], a["lda"], a["b"], a["ldb"], a["out"], a["ldo"], a["npix"], a["C"], a["slope"], None)

    def add_act_bwd(**kw):
        a = dict(dict(a=P, lda=8, b=P, ldb=8, out=P, ldo=8, npix=5, C=8, slope=0.0), **kw)
        return h.stem_add_act_bwd(a["a"], a["lda"], a["b"], a["ldb"], a["out"], a["ldo"], a["npix"], a["C"], a["slope"], None)

    def gate_fwd(**kw):
        a = dict(dict(a=P, lda=8, b=P, ldb=8, x=P, ldx=8, out=P, ldo=8, npix=5, C=8), **kw)
        return h.stem_gate_fwd(a["a"], a["lda"], a["b"], a["ldb"], a["x"], a["ldx"], a["out"], a["ldo"], a["npix"], a["C"], None)

    def gate_bwd(**kw):
        a = dict(dict(a=P, lda=8, b=P, ldb=8, x=P, ldx=8, out=P, ldo=8, db=P, lddb=8, npix=5, C=8), **kw)
        return h.stem_gate_bwd(a["a"], a["lda"], a["b"], a["ldb"], a["x"], a["ldx"], a["out"], a["ldo"], a["db"], a["lddb"], a["npix"],
                               a["C"], None)
    return {"stem_add_act_fwd": (add_act_fwd, ("a", "b", "out")), "stem_add_act_bwd": (add_act_bwd, ("a", "b", "out")),
            "stem_gate_fwd": (gate_fwd, ("a", "b", "x", "out")), "stem_gate_bwd": (gate_bwd, ("a", "b", "x", "out", "db"))}


@pytest.mark.parametrize("name", ["stem_add_act_fwd", "stem_add_act_bwd", "stem_gate_fwd", "stem_gate_bwd"])
def test_elementwise_argument_errors(name):
    h = _lib().hip()
    call, tensors = _elementwise_calls(h)[name]
    lds = {"a": "lda", "b": "ldb", "x": "ldx", "out": "ldo", "db": "lddb"}
    cases = [dict(C=0), dict(C=-1)]
    for t in tensors:
        cases += [{t: None}, {lds[t]: 7}, {lds[t]: 10}, {t: P + 4}, {"C": 3, lds[t]: 2}]
    for bad in cases:
        assert call(**bad) != 0 and name.encode() in h.stem_last_error(), (name, bad, h.stem_last_error())
    assert call(npix=0) == 0                                            # empty: nothing launched
    assert call(npix=0, C=3, **{lds[t]: 5 for t in tensors}) == 0       # C % 4 != 0: any pitch >= C
    assert call(npix=0, **{lds[t]: 12 for t in tensors}) == 0           # channel-slice views
