"""CPU: the C ABI of the validation glue (include/stem_validation.h: stem_eb_forward_eval_rate, stem_gc_forward_eval_rate,
stem_em_loss_accumulate; csrc/entropy.hip).  Argument errors name their function and are reported before anything touches a device, so
all of this runs without one."""
import ctypes as C
import os
import subprocess

NEW = ("stem_eb_forward_eval_rate", "stem_em_loss_accumulate", "stem_gc_forward_eval_rate")
NARGS = {"stem_eb_forward_eval_rate": 11, "stem_gc_forward_eval_rate": 12, "stem_em_loss_accumulate": 9}
P = 4096                      # a 16-byte aligned "pointer": never dereferenced, every call below returns before a launch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "stem_validation.h")
OTHER_HEADERS = ("stem_hip.h", "stem_ar_batch.h", "stem_blocks.h", "stem_hyperprior.h", "stem_eb_filters.h", "stem_gdn1.h")


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def test_the_header_parses_and_is_bound_off_the_tape():
    """include/stem_validation.h is read and bound like stem_gdn1.h; its entry points are additive (the ABI version stays 5, stem_hip.h
    keeps its 146 entry points) and outside the launch tape's table"""
    from spatiotemporalentropymodel_amd import _abi
    lib = _lib()
    protos = _abi.prototypes(HEADER)
    assert lib.declared_hip_validation_symbols() == sorted(NEW) == sorted(protos)
    assert {n: len(a) for n, (_, a) in protos.items()} == NARGS
    v, i, z, f, d = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_double
    assert protos["stem_eb_forward_eval_rate"] == (i, [v, i, v, v, v, v, v, z, i, f, v])
    assert protos["stem_gc_forward_eval_rate"] == (i, [v, v, v, i, v, v, v, z, i, f, f, v])
    assert protos["stem_em_loss_accumulate"] == (i, [v, i, v, i, d, d, v, v, v])
    others = set()
    for h in OTHER_HEADERS:
        others |= set(_abi.prototypes(os.path.join(REPO, "include", h)))
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


def test_the_library_exports_exactly_what_the_header_declares():
    """the dynamic symbol table of libstem_hip.so: every stem_* name that mentions the validation glue is one of the three, and the
    three are there"""
    lib = _lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.HIP_SO]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW) <= exported
    assert {n for n in exported if "eval_rate" in n or "em_loss_accumulate" in n} == set(NEW)
    declared = set(NEW)
    from spatiotemporalentropymodel_amd import _abi
    for h in OTHER_HEADERS:
        declared |= set(_abi.prototypes(os.path.join(REPO, "include", h)))
    assert {n for n in exported if n.startswith("stem_")} == declared, {n for n in exported if n.startswith("stem_")} ^ declared


def _eb(h, **kw):
    a = dict(dict(z=P, ldz=8, pack=P, medians=P, z_hat=P, lik=P, partials=P, npix=5, C=8), **kw)
    return h.stem_eb_forward_eval_rate(a["z"], a["ldz"], a["pack"], a["medians"], a["z_hat"], a["lik"], a["partials"], a["npix"], a["C"], 1e-9,
                                       None)


def _gc(h, **kw):
    a = dict(dict(y=P, scales=P, means=P, ldsm=16, out=P, lik=P, partials=P, npix=5, C=8), **kw)
    return h.stem_gc_forward_eval_rate(a["y"], a["scales"], a["means"], a["ldsm"], a["out"], a["lik"], a["partials"], a["npix"], a["C"], 0.11,
                                       1e-9, None)


def _acc(h, **kw):
    a = dict(dict(py=P, ny=3, pz=P, nz=2, out3=P, acc4=P), **kw)
    return h.stem_em_loss_accumulate(a["py"], a["ny"], a["pz"], a["nz"], -0.5, 1.0, a["out3"], a["acc4"], None)


def test_argument_errors_name_the_function():
    h = _lib().hip()
    cases = {"stem_eb_forward_eval_rate": (_eb, [dict(z=None), dict(pack=None), dict(medians=None), dict(z_hat=None), dict(lik=None),
                                                 dict(partials=None), dict(C=0), dict(C=-8), dict(ldz=7), dict(C=0, npix=0)]),
             "stem_gc_forward_eval_rate": (_gc, [dict(y=None), dict(scales=None), dict(means=None), dict(out=None), dict(lik=None),
                                                 dict(partials=None), dict(C=0), dict(C=-8), dict(ldsm=7), dict(C=0, npix=0)]),
             "stem_em_loss_accumulate": (_acc, [dict(acc4=None), dict(py=None), dict(pz=None), dict(ny=-1), dict(nz=-1)])}
    for name, (call, bad) in cases.items():
        for kw in bad:
            assert call(h, **kw) == -1 and name.encode() in h.stem_last_error(), (name, kw, h.stem_last_error())


def test_empty_tensors_launch_nothing():
    """npix == 0 with valid pointers and sizes: 0 without a launch (no device here), as the training twins answer"""
    h = _lib().hip()
    assert _eb(h, npix=0) == 0 and _gc(h, npix=0) == 0
    assert _eb(h, npix=0, z=None) == -1 and _gc(h, npix=0, y=None) == -1
