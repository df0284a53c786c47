"""CPU: include/stem_tail.h and libstem_tail.so (the optimiser pass over a table of chunk ranges): read, bound, exported by a library
of its own and recordable by a launch tape through that library's own table, apart from stem_hip.h's; argument errors; and the
chunk assignment of the ordered tail (engine.tail_chunk_ranges)."""
import ctypes as C
import os
import re
import subprocess
import sys

from conftest import REPO

NAME = "stem_adam_step_bmax_ranges"
ALL = [NAME, "stem_tail_entry_recordable", "stem_tail_last_error"]


def test_the_header_parses_is_bound_and_recordable():
    from spatiotemporalentropymodel_amd import _abi, _lib
    protos = _abi.prototypes(os.path.join(REPO, "include", "stem_tail.h"))
    assert sorted(protos) == ALL == _lib.declared_tail_symbols()
    assert not set(ALL) & set(_lib.declared_hip_symbols())
    v, i, z, f = C.c_void_p, C.c_int, C.c_size_t, C.c_float
    # stem_adam_step_bmax's arguments with (ranges, nranges) in front of the stream
    assert protos[NAME] == (i, [v, v, v, v, z, v, f, f, f, f, f, f, i, i, v, v, i, v])
    hip = dict(_lib._HIP_PROTO)["stem_adam_step_bmax"]
    assert protos[NAME][1][:15] == hip[1][:15] and protos[NAME][1][-1] is hip[1][-1]
    assert protos["stem_tail_last_error"] == (C.c_char_p, []) and protos["stem_tail_entry_recordable"] == (i, [v])
    assert _lib._TAPE_SIG[NAME] == protos[NAME][1] and set(_lib._TAPE_SIG) == set(_lib._HIP_SIG) | {NAME}
    assert subprocess.call([sys.executable, os.path.join(REPO, "tools", "gen_tape_table.py"), "--check"]) == 0
    csrc = os.path.join(REPO, "spatiotemporalentropymodel_amd", "csrc")
    assert re.findall(r"STEM_TAPE_ENTRY\((\w+)\)", open(os.path.join(csrc, "tape_entries_tail.inc")).read()) == ALL[:2]
    assert NAME not in open(os.path.join(csrc, "tape_entries.inc")).read()
    # a library of its own: it exports exactly the header, libstem_hip.so none of it
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.TAIL_SO]).decode()
    assert sorted(n for n in (line.split()[-1] for line in out.splitlines() if line.strip()) if n.startswith("stem_")) == ALL
    raw_hip = C.CDLL(_lib.HIP_SO)
    assert not any(hasattr(raw_hip, n) for n in ALL)
    lib, raw = _lib.tail(), C.CDLL(_lib.TAIL_SO)
    fn = getattr(lib, NAME)
    assert fn.restype is i and fn.argtypes == protos[NAME][1]
    addr = C.cast(getattr(raw, NAME), v).value
    assert lib.stem_tail_entry_recordable(addr) == 1 and _lib.hip().stem_tape_entry_recordable(addr) == 0
    assert lib.stem_tail_entry_recordable(C.cast(raw.stem_tail_last_error, v).value) == 0
    assert lib.stem_tail_entry_recordable(C.cast(raw_hip.stem_adam_step_bmax, v).value) == 0


def test_argument_errors_come_before_any_launch():
    """no device is touched: null pointers, a step count of 0, too many ranges and a range outside the buffer's chunks are refused
    with the function named"""
    from spatiotemporalentropymodel_amd import _lib
    lib = _lib.tail()
    ch = _lib.hip().stem_adam_chunk()
    P = 0x1000
    tab = (C.c_int * 2)(0, 2)
    args = lambda **kw: tuple(dict(dict(p=P, g=P, m=P, v=P, n=ch + 1, sumsq=None, a=0.0, b=1.0, c=1e-3, d=0.9, e=0.999, f=1e-8, step=1, zg=0,
                                        bmax=P, ranges=tab, nr=1, st=None), **kw).values())
    for bad in (dict(p=None), dict(bmax=None), dict(step=0), dict(nr=41), dict(nr=-1), dict(ranges=(C.c_int * 2)(1, 3)),
                dict(ranges=(C.c_int * 2)(2, 1)), dict(ranges=(C.c_int * 2)(-1, 1)), dict(ranges=None)):
        assert lib.stem_adam_step_bmax_ranges(*args(**bad)) < 0, bad
        assert NAME.encode() in lib.stem_tail_last_error(), bad
    # nothing to do: no launch, no error
    assert lib.stem_adam_step_bmax_ranges(*args(nr=0, ranges=None)) == 0
    assert lib.stem_adam_step_bmax_ranges(*args(ranges=(C.c_int * 2)(1, 1))) == 0
    assert lib.stem_adam_step_bmax_ranges(*args(n=0)) == 0


def test_launches_of_one_step_share_one_binding():
    """tape.LaunchTape.bind_floats: the same provider bound again follows the first binding (one optimiser step in several launches
    counts once); another provider is a binding of its own"""
    from spatiotemporalentropymodel_amd.tape import LaunchTape
    t = LaunchTape()
    call = lambda: t.entries.append(("call", "x", 0, [0, 1, 1], [0, 0, 0], [0.0, 0.0, 0.0], [], [False] * 3))
    a, b = (lambda: (1.0, 2.0)), (lambda: (3.0, 4.0))
    for prov in (a, None, a, b, a):
        call()
        if prov is not None:
            t.bind_floats(prov)
    assert t.float_bindings == {0: a, 3: b} and t.float_followers == {2: 0, 4: 0}
    assert t._provider(4) is a and t._provider(3) is b and sorted(t._bound_entries()) == [0, 2, 3, 4]


def test_chunk_ranges_cover_every_chunk_once():
    from spatiotemporalentropymodel_amd.engine import tail_chunk_ranges
    # (offset, elements, group): a group-2 tensor whose first chunk is shared with group 0 and whose last with group 1
    tensors = [(0, 100, 0), (100, 3 * 64, 2), (292, 10, 1), (304, 200, 3)]
    r = tail_chunk_ranges(tensors, 504, 64, 4)
    assert r == [[(0, 2)], [(4, 5)], [(2, 4)], [(5, 8)]]
    # the bench model's layout: every chunk exactly once, each table within the 40 ranges of one call
    import torch
    from spatiotemporalentropymodel_amd import optim
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    with torch.device("meta"):
        m = SpatioTemporalPriorModel_Res()
    named = sorted(((n, p) for n, p in m.named_parameters() if not n.endswith(".quantiles")), key=lambda t: optim.backward_layout_key(t[0]))
    group = {"TPM.0.weight": 0, "HE.0.weight": 0, "TPM.2.weight": 1, "HE.2.weight": 1, "TPM.4.weight": 2, "HE.4.weight": 2}
    tensors, off = [], 0
    for n, p in named:
        is_layer = n.endswith(".weight") and p.dim() == 4
        tensors.append((off, p.numel(), group.get(n, 3) if is_layer else 0))
        off += (p.numel() + 3) // 4 * 4
    r = tail_chunk_ranges(tensors, off, 4096, 4)
    chunks = sorted(c for g in r for a, b in g for c in range(a, b))
    assert chunks == list(range((off + 4095) // 4096)) and all(0 < len(g) <= 40 for g in r)
    sizes = [sum(b - a for a, b in g) * 4096 for g in r]
    assert sizes[0] < 2.5e6 and sizes[3] > 7e6            # the first group is TPM.0 + HE.0 and the chunks of the small tensors, no more
