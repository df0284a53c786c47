"""CPU: the C ABI of the zero-mean likelihood kernels (include/stem_hyperprior.h: stem_gc_scale_forward / _backward, stem_abs_fwd / _bwd;
csrc/hyperprior.hip).  Argument errors name their function and are reported before anything touches a device, and empty calls return
0 without a launch, so all of this runs without one."""
import ctypes as C
import os

import pytest

NEW = ("stem_gc_scale_forward", "stem_gc_scale_backward", "stem_abs_fwd", "stem_abs_bwd")
NARGS = {"stem_gc_scale_forward": 20, "stem_gc_scale_backward": 18, "stem_abs_fwd": 7, "stem_abs_bwd": 9}
P = 4096                      # a 16-byte aligned "pointer": never dereferenced, every call below returns before a launch


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def test_symbols_are_declared_bound_and_off_the_tape():
    """include/stem_hyperprior.h is read and bound like stem_blocks.h; its entry points are additive (the ABI version stays 5) and
    outside the launch tape's table, which lists stem_hip.h's entry points"""
    from spatiotemporalentropymodel_amd import _abi
    lib = _lib()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    protos = _abi.prototypes(os.path.join(repo, "include", "stem_hyperprior.h"))
    assert lib.declared_hip_hyperprior_symbols() == sorted(NEW) == sorted(protos)
    assert {n: len(a) for n, (_, a) in protos.items()} == NARGS and all(r is C.c_int for r, _ in protos.values())
    assert protos["stem_gc_scale_forward"][1][4:8] == [C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]      # seed, offset, epoch, stride
    assert protos["stem_abs_fwd"][1] == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_void_p]
    others = set(lib.declared_hip_symbols()) | set(lib.declared_hip_batch_symbols()) | set(lib.declared_hip_block_symbols())
    assert not set(NEW) & others
    assert len(lib.declared_hip_symbols()) == 146                      # stem_hip.h, and with it the tape's table, is untouched
    raw = C.CDLL(lib.HIP_SO)
    h = lib.hip()
    assert h.stem_abi_version() == 5
    for name in NEW:
        fn = getattr(h, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == NARGS[name], name
        assert h.stem_tape_entry_recordable(C.cast(getattr(raw, name), C.c_void_p)) == 0, name
    text = open(os.path.join(repo, "spatiotemporalentropymodel_amd", "csrc", "tape_entries.inc")).read()
    assert not any(name in text for name in NEW)


def _forward(h, **kw):
    a = dict(dict(y=P, ldy=8, noise=P, ldn=8, scales=P, lds=8, out=P, ldo=8, lik=P, ldl=8, npix=5, C=8, mode=0), **kw)
    return h.stem_gc_scale_forward(a["y"], a["ldy"], a["noise"], a["ldn"], 1, 2, None, 0, a["scales"], a["lds"], a["out"], a["ldo"], a["lik"],
                                   a["ldl"], a["npix"], a["C"], a["mode"], 0.11, 1e-9, None)


def _backward(h, **kw):
    a = dict(dict(out=P, ldo=8, scales=P, lds=8, dlik=P, ldl=8, dout=P, ldg=8, dscales=P, ldds=8, dy=P, lddy=8, npix=5, C=8, q=None), **kw)
    return h.stem_gc_scale_backward(a["out"], a["ldo"], a["scales"], a["lds"], a["dlik"], a["ldl"], a["dout"], a["ldg"], a["dscales"], a["ldds"],
                                    a["dy"], a["lddy"], a["npix"], a["C"], 0.11, 1e-9, a["q"], None)


def _abs_fwd(h, **kw):
    a = dict(dict(x=P, ldx=8, out=P, ldo=8, npix=5, C=8), **kw)
    return h.stem_abs_fwd(a["x"], a["ldx"], a["out"], a["ldo"], a["npix"], a["C"], None)


def _abs_bwd(h, **kw):
    a = dict(dict(x=P, ldx=8, g=P, ldg=8, dx=P, lddx=8, npix=5, C=8), **kw)
    return h.stem_abs_bwd(a["x"], a["ldx"], a["g"], a["ldg"], a["dx"], a["lddx"], a["npix"], a["C"], None)


CALLS = {"stem_gc_scale_forward": (_forward, (dict(y=None), dict(scales=None), dict(out=None), dict(lik=None), dict(mode=2), dict(mode=-1),
                                              dict(C=0), dict(C=-4), dict(ldy=7), dict(ldn=7), dict(lds=7), dict(ldo=7), dict(ldl=7),
                                              dict(C=3, lds=2))),
         "stem_gc_scale_backward": (_backward, (dict(out=None), dict(scales=None), dict(dlik=None), dict(dy=None), dict(C=0), dict(ldo=7),
                                                dict(lds=7), dict(ldl=7), dict(ldg=7), dict(ldds=7), dict(lddy=7))),
         "stem_abs_fwd": (_abs_fwd, (dict(x=None), dict(out=None), dict(C=0), dict(ldx=7), dict(ldo=7))),
         "stem_abs_bwd": (_abs_bwd, (dict(x=None), dict(g=None), dict(dx=None), dict(C=-1), dict(ldx=7), dict(ldg=7), dict(lddx=7)))}


@pytest.mark.parametrize("name", NEW)
def test_argument_errors_name_the_function(name):
    h = _lib().hip()
    call, cases = CALLS[name]
    for bad in cases:
        assert call(h, **bad) == -1 and name.encode() in h.stem_last_error(), (name, bad, h.stem_last_error())
    assert b"smaller than C" in (call(h, **{k: v for k, v in cases[-1].items()}), h.stem_last_error())[1]


@pytest.mark.parametrize("name", NEW)
def test_empty_calls_return_zero_without_a_launch(name):
    """npix == 0: 0, whatever else is passed -- null pointers, odd pitches, odd alignment (nothing is launched, so no device is needed)"""
    h = _lib().hip()
    call, _ = CALLS[name]
    assert call(h, npix=0) == 0
    assert call(h, npix=0, C=3) == 0
    if name == "stem_gc_scale_forward":
        assert call(h, npix=0, y=None, noise=None, scales=None, out=None, lik=None) == 0 and call(h, npix=0, mode=1, noise=None, lds=12) == 0
    elif name == "stem_gc_scale_backward":
        assert call(h, npix=0, out=None, scales=None, dlik=None, dout=None, dscales=None, dy=None) == 0
    else:
        assert call(h, npix=0, x=None) == 0
