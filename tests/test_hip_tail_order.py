"""GPU: the optimiser tail of the fused P-frame step in first-use order (engine.StemEngine.tail_plan / run_tail).

The order of the launches changes, no number does: stem_adam_step_bmax_ranges over tables of chunk ranges leaves what one
stem_adam_step_bmax pass leaves, and four P-frame steps with the ordered tail -- the later groups on the weight-gradient stream,
under the next forward -- leave the bytes the single pass + single pair pack leave, on the fused and on the taped route, also when
the weight-gradient stream is held back so that only the groups' events keep a consumer from stale images."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bytes_equal(a, b):
    return (a.dtype == b.dtype and a.shape == b.shape
            and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))


# ---- test 1: op level ------------------------------------------------------------------------------------------------------------

#: the six chunks of the buffer below dealt to three tables in permuted order: a single-chunk range, the ragged last chunk (5)
TABLES = ([(4, 5), (1, 2)], [(5, 6)], [(2, 4), (0, 1)])


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("clip", [False, True])
def test_adam_ranges_equals_one_pass(clip, zero_grad, step):
    from spatiotemporalentropymodel_amd import functional as F
    ch = F.adam_chunk()
    n = 5 * ch + 37
    rng = np.random.default_rng(3)
    host = {"p": rng.standard_normal(n) * 0.05, "g": rng.standard_normal(n) * np.exp(rng.uniform(-12, 2, n)),
            "m": rng.standard_normal(n) * 1e-3, "v": rng.standard_normal(n) ** 2 * 1e-4}
    acc = None
    if clip:                                        # the norm is above max_norm = 1: the clip coefficient scales every gradient
        acc = F.sumsq_accumulator(torch.device("cuda:0"))
        F.sumsq(torch.tensor(host["g"].astype(np.float32), device="cuda"), acc, overwrite=True)
        assert float(acc[0]) > 1.0
    args = (acc, 1.0 if clip else 0.0, 0.5, 1e-3, 0.9, 0.999, 1e-8, step)
    runs = []
    for ranged in (False, True):
        t = {k: torch.tensor(a.astype(np.float32), device="cuda") for k, a in host.items()}
        bmax = torch.full((4 * ((n + ch - 1) // ch),), -1.0, device="cuda")
        if ranged:
            for tab in TABLES:
                F.adam_step_bmax_ranges(t["p"], t["g"], t["m"], t["v"], *args, bmax, F.adam_ranges(tab), zero_grad=zero_grad)
        else:
            F.adam_step_bmax(t["p"], t["g"], t["m"], t["v"], *args, bmax, zero_grad=zero_grad)
        runs.append(dict(t, bmax=bmax))
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "g", "bmax"):
        assert _bytes_equal(runs[0][k], runs[1][k]), k
    assert float(runs[1]["bmax"].min()) >= 0.0                                 # every slot written, the ragged chunk's too
    assert not _bytes_equal(runs[1]["p"], torch.tensor(host["p"].astype(np.float32), device="cuda"))
    assert (float(runs[1]["g"].abs().max()) == 0.0) == zero_grad


def test_adam_ranges_touches_only_its_chunks():
    from spatiotemporalentropymodel_amd import functional as F
    ch = F.adam_chunk()
    n = 5 * ch + 37
    g0 = torch.Generator(device="cuda").manual_seed(1)
    p, g, m, v = (torch.randn(n, device="cuda", generator=g0) for _ in range(4))
    v.abs_()
    before = [t.clone() for t in (p, g, m, v)]
    bmax = torch.full((4 * 6,), -1.0, device="cuda")
    F.adam_step_bmax_ranges(p, g, m, v, None, 0.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1, bmax, F.adam_ranges([(3, 4), (3, 3), (5, 6)]), zero_grad=True)
    torch.cuda.synchronize()
    touched = torch.zeros(n, dtype=torch.bool, device="cuda")
    touched[3 * ch:4 * ch] = True
    touched[5 * ch:] = True
    for t, b in zip((p, g, m, v), before):
        assert torch.equal(t[~touched], b[~touched]) and not torch.equal(t[touched], b[touched])
    assert (bmax.view(6, 4)[[0, 1, 2, 4]] == -1.0).all() and (bmax.view(6, 4)[[3, 5]] >= 0.0).all()
    with pytest.raises(RuntimeError):
        F.adam_step_bmax_ranges(p, g, m, v, None, 0.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1, bmax, F.adam_ranges([(5, 7)]))


# ---- tests 2-4: step level -------------------------------------------------------------------------------------------------------

STEPS = 4


def _run(route, ordered, hook=False, sync=True):
    """four consecutive P-frame steps of SpatioTemporalPriorModel_Res(64, 96) on B = 2, 16 x 16 latents -> per step the bytes the
    step leaves.  sync=True: finish() after every step, then parameters, moments, every packed image with its scale record, the
    losses, the auxiliary loss and the gradient norm.  sync=False: nothing orders the compute stream after the auxiliary stream
    between two steps (only what the schedule itself enqueues); per step the losses and y_hat, the rest after the last step."""
    from spatiotemporalentropymodel_amd import selfcheck as S
    from spatiotemporalentropymodel_amd import trainer
    from spatiotemporalentropymodel_amd.optim import configure_optimizers
    from spatiotemporalentropymodel_amd.tape import TapedPFrameStep
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    _, stem = S.build_models(64, 96, 64, 96, dev, closed_form=False, inject_noise=False)
    stem.train()
    opt, aux = configure_optimizers(stem, types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3))
    eng = stem.engine()
    eng.tail_ordered = ordered
    if hook:
        eng.tail_hook = lambda: torch.cuda._sleep(25_000_000)        # ~11 ms (measured: 0.45 ms per 10^6 cycles of the spin kernel's counter)
    fused = trainer.FusedPFrameStep(stem, opt, aux)
    step = TapedPFrameStep(fused) if route == "taped" else fused
    steps = STEPS + (4 if route == "taped" else 0)                   # taped: two ordinary, two recorded, then four replays
    g = torch.Generator(device=dev).manual_seed(4)
    ys = [torch.randn(2, 96, 16, 16, device=dev, generator=g) * 3.0 for _ in range(steps + 1)]
    y_cond, log, lazy = ys[0], [], []
    torch.cuda.synchronize()

    def state():
        rec = {"p": opt.flat.data.clone(), "m": opt.m.clone(), "v": opt.v.clone(), "aux_p": aux.flat.data.clone()}
        for i, l in enumerate(eng.layers):
            for role, img in (("fwd", l.wp6_fwd), ("dgrad", l.wp6_dgrad)):
                if img is not None:
                    rec[f"img{i}{role}"] = img.clone()
        return rec

    for t in range(1, steps + 1):
        out, oc, aux_l, gn = step.step(ys[t], y_cond, 2 * 256 * 256)
        y_cond = out["y_hat"].clone()
        assert (fused._tail_plan is not None) == ordered
        if t <= steps - STEPS:
            continue
        rec = {"y_hat": y_cond, "loss": torch.stack([oc["y_bpp_loss"], oc["z_bpp_loss"], oc["loss"]])}
        if sync:
            step.finish()                                            # the reader's side of the contract: parameters are read after it
            rec.update(state(), aux=aux_l.tensor().clone(), gn=gn.tensor().clone())
        else:
            lazy.append((aux_l, gn))                                 # (reading them would make this stream wait for the auxiliary one)
        log.append(rec)
    if not sync:
        step.finish()
        log[-1].update(state())
        for rec, (aux_l, gn) in zip(log, lazy):
            rec.update(aux=aux_l.tensor().clone(), gn=gn.tensor().clone())
    torch.cuda.synchronize()
    if route == "taped":
        assert step.tape is not None and step.replays >= STEPS
    return log


_RUNS = {}


def _cached(*key):
    if key not in _RUNS:
        _RUNS[key] = _run(*key)
    return _RUNS[key]


def _assert_same(a, b):
    assert len(a) == len(b) == STEPS
    for t, (ra, rb) in enumerate(zip(a, b)):
        assert ra.keys() == rb.keys() and {"loss", "aux", "gn", "y_hat"} <= ra.keys()
        for k in ra:
            assert _bytes_equal(ra[k], rb[k]), (t, k)
    assert sum(k.startswith("img") for k in a[-1]) >= 20 and "p" in a[-1]


def test_ordered_tail_changes_no_byte_fused():
    _assert_same(_cached("fused", False), _cached("fused", True))


def test_ordered_tail_changes_no_byte_taped():
    """... and the replayed steps (the waits cross the step boundary inside the tape) against the single pass on the same route"""
    _assert_same(_cached("taped", False), _cached("taped", True))


def test_consumers_wait_for_their_group():
    """the weight-gradient stream held back for ~10 ms in front of the later groups, and nothing but the schedule's own events
    between two steps: the next forward's kernels are enqueued long before the groups have run, and only the groups' events keep
    them from the previous step's images (a stale image shows in the next step's losses).  Against the single pass, unheld."""
    ref = _cached("fused", False, False, False)
    _assert_same(ref, _cached("fused", True, False, False))
    _assert_same(ref, _cached("fused", True, True, False))


def test_parameters_after_finish_are_the_updated_ones():
    """finish() orders the current stream after every group: opt.flat.data read right after it is the single pass's, after every
    step and with the later groups held back"""
    for ref, run in ((_cached("fused", False), _cached("fused", True)), (_cached("fused", False, False, False), _cached("fused", True, True, False))):
        for ra, rb in zip(ref, run):
            for k in ("p", "m", "v"):
                assert (k in ra) == (k in rb) and (k not in ra or _bytes_equal(ra[k], rb[k]))
    assert all("p" in r for r in _cached("fused", True)) and "p" in _cached("fused", True, True, False)[-1]
