"""CPU: the C ABI of the EntropyBottleneck kernels for any `filters` tuple (include/stem_eb_filters.h, csrc/eb_filters.hip), the host
arithmetic of functional.ebf_layout / ebf_nparam, and the constructor's refusals.  Argument errors are reported before anything touches
a device, so all of this runs without one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eb_filters_ref as ebr
import entropy_ref as er

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "stem_eb_filters.h")
NEW = ("stem_ebf_nparam", "stem_ebf_pack", "stem_ebf_unpack_grads", "stem_ebf_forward", "stem_ebf_backward", "stem_ebf_aux_loss_grad")
NARGS = {"stem_ebf_nparam": 2, "stem_ebf_pack": 6, "stem_ebf_unpack_grads": 7, "stem_ebf_forward": 16, "stem_ebf_backward": 14,
         "stem_ebf_aux_loss_grad": 10}
P = 4096                      # a "pointer": never dereferenced, every call below returns before a launch
NPARAM = {(): 2, (1,): 5, (1, 1): 8, (5,): 21, (3, 3, 3): 43, (3, 3, 3, 3): 58, (2, 4, 8): 79, (3,) * 6: 88, (8,) * 6: 433}
BAD = ((3,) * 7, (0,), (9,), (3, -1, 3), (3, 0), (8, 8, 8, 9))


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def _ints(filters):
    return ((C.c_int * len(filters))(*filters) if filters else None), len(filters)


def test_symbols_are_declared_bound_and_off_the_tape():
    """the header is read by _abi.prototypes and bound like stem_blocks.h / stem_hyperprior.h; libstem_hip.so exports every declared
    symbol; the entry points are additive (the ABI version stays 5) and outside the launch tape's table"""
    from spatiotemporalentropymodel_amd import _abi
    lib = _lib()
    protos = _abi.prototypes(HEADER)
    assert lib.declared_hip_eb_filters_symbols() == sorted(NEW) == sorted(protos)
    assert {n: len(a) for n, (_, a) in protos.items()} == NARGS and all(r is C.c_int for r, _ in protos.values())
    assert protos["stem_ebf_nparam"][1] == [C.c_void_p, C.c_int]
    assert protos["stem_ebf_pack"][1] == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    others = (set(lib.declared_hip_symbols()) | set(lib.declared_hip_batch_symbols()) | set(lib.declared_hip_block_symbols()) |
              set(lib.declared_hip_hyperprior_symbols()))
    assert not set(NEW) & others
    assert len(lib.declared_hip_symbols()) == 146                      # stem_hip.h, and with it the tape's table, is untouched
    raw = C.CDLL(lib.HIP_SO)
    h = lib.hip()
    assert h.stem_abi_version() == 5
    for name in NEW:
        fn = getattr(h, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == NARGS[name], name
        assert h.stem_tape_entry_recordable(C.cast(getattr(raw, name), C.c_void_p)) == 0, name
    text = open(os.path.join(REPO, "spatiotemporalentropymodel_amd", "csrc", "tape_entries.inc")).read()
    assert not any(name in text for name in NEW)


def test_caps_macros_equal_the_python_constants():
    from spatiotemporalentropymodel_amd import functional as F
    macros = {k: int(v) for k, v in re.findall(r"^#define\s+(STEM_EBF_\w+)\s+(\d+)", open(HEADER).read(), flags=re.M)}
    assert macros == {"STEM_EBF_MAX_FILTERS": F.EBF_MAX_FILTERS, "STEM_EBF_MAX_WIDTH": F.EBF_MAX_WIDTH, "STEM_EBF_MAX_NPARAM": F.EBF_MAX_NPARAM}
    assert (F.EBF_MAX_FILTERS, F.EBF_MAX_WIDTH, F.EBF_MAX_NPARAM) == (ebr.MAX_FILTERS, ebr.MAX_WIDTH, ebr.MAX_NPARAM) == (6, 8, 433)
    assert F.ebf_nparam((F.EBF_MAX_WIDTH,) * F.EBF_MAX_FILTERS) == F.EBF_MAX_NPARAM


@pytest.mark.parametrize("filters", sorted(NPARAM), ids=ebr.tuple_id)
def test_layout_matches_the_numpy_statement(filters):
    """F.ebf_layout / F.ebf_nparam / stem_ebf_nparam against eb_filters_ref.layout; (3, 3, 3, 3) is today's [C][58] image, offset for
    offset (entropy_ref.EB_OFF / EB_LEN == kOff / kLen of csrc/entropy.hip)"""
    from spatiotemporalentropymodel_amd import functional as F
    want = [(name, off, n) for name, _, off, n in ebr.layout(filters)]
    assert F.ebf_layout(filters) == want and len(want) == 3 * len(filters) + 2
    assert F.ebf_nparam(filters) == ebr.nparam(filters) == NPARAM[filters] == _lib().hip().stem_ebf_nparam(*_ints(filters))
    assert F.ebf_tensor_names(filters) == [name for name, _, _ in want]
    if filters == (3, 3, 3, 3):
        assert [name for name, _, _ in want] == F.EB_TENSORS == er.EB_NAMES
        assert [off for _, off, _ in want] == er.EB_OFF and [n for _, _, n in want] == er.EB_LEN and F.ebf_nparam(filters) == F.EB_NPARAM


def _calls(h, fa, nf, **kw):
    a = dict(dict(p=P, C=5), **kw)
    p, Cc = a["p"], a["C"]
    return {"stem_ebf_pack": lambda: h.stem_ebf_pack(p, fa, nf, p, Cc, None),
            "stem_ebf_unpack_grads": lambda: h.stem_ebf_unpack_grads(p, p, fa, nf, Cc, 0, None),
            "stem_ebf_forward": lambda: h.stem_ebf_forward(p, Cc, p, p, p, fa, nf, p, p, 1, 2, 3, Cc, 0, 1e-9, None),
            "stem_ebf_backward": lambda: h.stem_ebf_backward(p, p, p, p, fa, nf, p, p, 1, 2, 3, Cc, 1e-9, None),
            "stem_ebf_aux_loss_grad": lambda: h.stem_ebf_aux_loss_grad(p, p, p, fa, nf, p, p, Cc, 0, None)}


@pytest.mark.parametrize("name", NEW[1:])
def test_refusals_come_before_any_launch(name):
    """too many filters, a width of 0 or 9 or below 0, a null filters array with n_filters > 0, n_filters < 0, null pointers, C <= 0:
    -1 with the function's name in stem_last_error(), and no device is touched (this test runs without one)"""
    h = _lib().hip()
    for bad in BAD:
        assert h.stem_ebf_nparam(*_ints(bad)) == -1
        assert _calls(h, *_ints(bad))[name]() == -1 and name.encode() in h.stem_last_error(), (name, bad, h.stem_last_error())
    for fa, nf in ((None, 2), (_ints((3, 3))[0], -1)):
        assert h.stem_ebf_nparam(fa, nf) == -1
        assert _calls(h, fa, nf)[name]() == -1 and name.encode() in h.stem_last_error()
    for kw in (dict(p=None), dict(C=0), dict(C=-3)):
        assert _calls(h, *_ints((3, 3, 3)), **kw)[name]() == -1 and name.encode() in h.stem_last_error(), (name, kw, h.stem_last_error())
    if name == "stem_ebf_forward":          # an empty tensor: 0, nothing launched;  a pitch below C: refused
        fa, nf = _ints((2, 4, 8))
        assert h.stem_ebf_forward(P, 5, P, P, P, fa, nf, P, P, 0, 2, 3, 5, 0, 1e-9, None) == 0
        assert h.stem_ebf_forward(P, 4, P, P, P, fa, nf, P, P, 1, 2, 3, 5, 0, 1e-9, None) == -1
        assert h.stem_ebf_forward(P, 5, None, P, P, fa, nf, P, P, 1, 2, 3, 5, 0, 1e-9, None) == -1 and b"noise" in h.stem_last_error()
        assert h.stem_ebf_forward(P, 5, P, P, None, fa, nf, P, P, 1, 2, 3, 5, 1, 1e-9, None) == -1 and b"medians" in h.stem_last_error()


def test_constructor_refusals_and_reference_keys(golden):
    """a tuple outside the caps: NotImplementedError naming both caps; a width below 1: ValueError; otherwise the module builds on the
    CPU with the reference's state-dict keys, order and shapes (tests/golden/eb_filters.npz)"""
    from spatiotemporalentropymodel_amd.entropy_models import EntropyBottleneck
    for bad in ((3,) * 7, (9,), (8, 8, 16)):
        with pytest.raises(NotImplementedError, match=r"at most 6 filters of width at most 8"):
            EntropyBottleneck(5, filters=bad)
    for bad in ((0,), (3, -1, 3), (3,) * 7 + (0,)):
        with pytest.raises(ValueError, match="filters"):
            EntropyBottleneck(5, filters=bad)
    g = golden("eb_filters.npz")
    for filters in ebr.GOLDEN_TUPLES:
        eb = EntropyBottleneck(int(g["C"][0]), filters=filters)
        assert eb.filters == filters
        assert [f"{k}|{','.join(map(str, v.shape))}" for k, v in eb.state_dict().items()] == list(g[f"{ebr.tuple_id(filters)}:names"])
        assert [n for n, _ in eb.named_parameters()][:-1] == [name for name, _, _, _ in ebr.layout(filters)]
    assert EntropyBottleneck(4)._tensors14()[0].shape == (4, 3, 1)
    with pytest.raises(ValueError, match="filters"):
        EntropyBottleneck(4, filters=(3, 3, 3))._tensors14()


def test_cpu_tensors_are_rejected():
    """there is no CPU route: every functional.ebf_* call refuses CPU tensors, as everywhere else"""
    from spatiotemporalentropymodel_amd import functional as F
    filters, Cc = (2, 4), 3
    lay = ebr.layout(filters)
    tensors = [torch.zeros(Cc, *shape) for _, shape, _, _ in lay]
    pack, x = torch.zeros(Cc, ebr.nparam(filters)), torch.zeros(1, Cc, 2, 2).contiguous(memory_format=torch.channels_last)
    q = torch.zeros(Cc, 1, 3)
    for call in (lambda: F.ebf_pack(tensors, filters), lambda: F.ebf_unpack_grads(pack, tensors, filters),
                 lambda: F.ebf_forward(x, pack, filters, noise=x), lambda: F.ebf_forward(x, pack, filters, medians=torch.zeros(Cc)),
                 lambda: F.ebf_backward(x, pack, x, filters), lambda: F.ebf_aux_loss_grad(q, pack, torch.zeros(3), filters, q.clone())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="outside the caps"):
        F.ebf_layout((9,))
