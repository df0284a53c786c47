"""GPU, two data-parallel ranks on ONE MI355X (BASELINE configs[2] / configs[4] at world size 2).

Two worker processes (tests/dp_worker.py, started by conftest.py at collection time) share cuda:0 and exchange through
gloo; each runs the real HIP forward / backward on ONE sample with the product's reducers attached:
  * `train`: distributed.OverlappedGradReducer hooked into StemEngine.backward (slices all-reduced from the
    weight-gradient stream while backward is still running), fused clip+Adam with grad_scale = 1/world;
  * `gop`:   distributed.GopGradAccumulator inside selfcheck.roi_gop_step (per-frame exchange, clip of the running sum).
This process then runs the SAME two samples as one batch of 2 on a single rank and compares: the reference has no
distributed code, so "correct" means "equals the single-device full-batch run", which the reference goldens
pin in test_hip_models.py / test_hip_roi.py.
"""
import types

import numpy as np
import pytest
import torch

from conftest import assert_close
from dp_worker import SlicedNoise, flat_np

pytestmark = pytest.mark.gpu


def _rel_to_rms(a, b):
    rms = float(np.sqrt(np.mean(np.square(b, dtype=np.float64)))) or 1.0
    return float(np.max(np.abs(a.astype(np.float64) - b)) / rms)


@pytest.mark.dp2("train")
def test_overlapped_reducer_two_ranks_equals_full_batch(dp2_results):
    from spatiotemporalentropymodel_amd import selfcheck as S
    from spatiotemporalentropymodel_amd.losses import EMLoss
    from spatiotemporalentropymodel_amd.optim import configure_optimizers
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    r0, r1 = dp2_results("train")
    # replicas: identical exchanged gradient and bit-identical parameters after two optimiser steps
    np.testing.assert_array_equal(r0["grad_avg"], r1["grad_avg"])
    np.testing.assert_array_equal(r0["params"], r1["params"])
    np.testing.assert_array_equal(r0["quantiles"], r1["quantiles"])
    # 5 contiguous runs per step (EPM, ctx, TPM, HD + bottleneck -- neighbours in the backward-ordered layout --, HE) x 2 steps
    assert int(r0["reducer_calls"][0]) == 10

    # single process, batch = the two ranks' samples
    dev = torch.device("cuda:0")
    steps = 2
    imodel, stem = S.build_models(64, 96, 64, 96, dev, inject_noise=False)
    stem.train()
    imodel.gaussian_conditional.noise_source = SlicedNoise("iframe_gc", 0, 1, 2)
    stem.entropy_bottleneck.noise_source = SlicedNoise("stem_eb", 0, 1, 2, batch_last=True)
    stem.gaussian_conditional.noise_source = SlicedNoise("stem_gc", 0, 1, 2)
    opt, aux_opt = configure_optimizers(stem, types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3))
    crit = EMLoss()
    frames = [f.to(dev) for f in smooth_frames("dp2:train", 2, steps + 1, 64)]
    with torch.no_grad():
        _, y_cond = imodel.getY(frames[0])
    for t in range(1, steps + 1):
        if t == 1:
            opt.zero_grad(), aux_opt.zero_grad()
            with torch.no_grad():
                y_cur, _ = imodel.getY(frames[t])
            out = stem(y_cur, y_cond)
            oc = crit(out, frames[t])
            oc["loss"].backward()
            grad_full = flat_np(opt.flat.grad)
            gn = opt.grad_norm()
            opt.step(norm_is_current=True)
            aux = stem.aux_loss()
            aux.backward()
            aux_opt.step()
        else:
            out, oc, aux, gn = S.p_frame_step(imodel, stem, crit, opt, aux_opt, frames[t], y_cond)
        y_cond = out["y_hat"]
        # EMLoss normalises by the local pixel count: the full-batch loss is the mean of the ranks' losses
        l0, l1 = r0[f"s{t}:loss"], r1[f"s{t}:loss"]
        assert abs(0.5 * (l0[0] + l1[0]) - float(oc["loss"])) <= 2e-6 * float(oc["loss"]), (t, l0, l1, float(oc["loss"]))
        assert l0[1] == l1[1] and abs(l0[1] - float(gn)) <= 1e-5 * float(gn), (t, l0[1], float(gn))    # norm of the averaged gradient
        assert l0[2] == l1[2] and abs(l0[2] - float(aux)) <= 1e-6 * abs(float(aux))
    # the averaged gradient of step 1, tensor by tensor (summation order differs: split-K over 1 vs 2 samples)
    worst = 0.0
    for name, p, o in zip(opt.flat.names, opt.flat.params, opt.flat.offsets):
        n = p.numel()
        worst = max(worst, _rel_to_rms(r0["grad_avg"][o:o + n], grad_full[o:o + n]))
        assert worst <= 2e-5, (name, worst)
    print(f"dp2 train: worst per-tensor |avg of rank gradients - full-batch gradient| / rms = {worst:.2e}")
    # parameters after two Adam steps: within fp32 rounding except elements whose gradient is noise around 0 (an Adam
    # step is lr * g / (|g| + eps): those may move the other way, at most 2 lr per step apart)
    pf = flat_np(opt.flat.data)
    err = np.abs(r0["params"].astype(np.float64) - pf)
    assert err.max() <= 4.2e-4, err.max()
    assert float((err <= 2e-6 * np.maximum(np.abs(pf), 1.0)).mean()) >= 0.98


@pytest.mark.dp2("train_fused")
@pytest.mark.dp2("train")
def test_fused_schedule_with_reducer_two_ranks_matches_generic_route(dp2_results):
    """`bench.py --gpus N` runs trainer.FusedPFrameStep with the overlapped reducer: two ranks of it must land where two ranks
    of the generic route (the `train` case, itself checked against the single-process full batch above) land."""
    f0, f1 = dp2_results("train_fused")
    g0, _ = dp2_results("train")
    np.testing.assert_array_equal(f0["grad_avg"], f1["grad_avg"])
    np.testing.assert_array_equal(f0["params"], f1["params"])
    np.testing.assert_array_equal(f0["quantiles"], f1["quantiles"])
    assert int(f0["reducer_calls"][0]) == 10
    scale = float(np.abs(g0["grad_avg"]).max())
    assert float(np.abs(f0["grad_avg"] - g0["grad_avg"]).max()) <= 2e-6 * scale        # coef / lik vs (1 / lik) * (g / ln 2)
    for t in (1, 2):
        a, b = f0[f"s{t}:loss"], g0[f"s{t}:loss"]
        assert abs(a[0] - b[0]) <= 1e-5 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-4 * b[1] and abs(a[2] - b[2]) <= 1e-5 * abs(b[2]), (t, a, b)
    # two Adam steps: elements whose gradient is fp32 noise may step the other way (<= 2 lr per step), the rest agree
    err = np.abs(f0["params"].astype(np.float64) - g0["params"])
    assert err.max() <= 4.2e-4 and float((err <= 2e-6 * np.maximum(np.abs(g0["params"]), 1.0)).mean()) >= 0.96


@pytest.mark.dp2("gop")
def test_gop_accumulator_two_ranks_equals_full_batch(dp2_results):
    from spatiotemporalentropymodel_amd import selfcheck as S
    from spatiotemporalentropymodel_amd.losses import PixelwiseRateDistortionLoss
    from spatiotemporalentropymodel_amd.models import stem_roi, stem_roi_i
    from spatiotemporalentropymodel_amd.optim import configure_optimizers
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_scaled_, closed_form_input, smooth_frames
    r0, r1 = dp2_results("gop")
    for k in ("params_i", "params_p", "grad_i", "grad_p"):
        np.testing.assert_array_equal(r0[k], r1[k])       # replicas stay bit-identical
    dev = torch.device("cuda:0")
    imodel = closed_form_fill_scaled_(stem_roi_i(), "stem_roi_i", 0.7).to(dev).train()
    pmodel = closed_form_fill_scaled_(stem_roi(), "stem_roi", 0.7).to(dev).train()
    for m, tag in ((imodel, "i"), (pmodel, "p")):
        m.entropy_bottleneck.noise_source = SlicedNoise(f"roi_{tag}_eb", 0, 1, 2, batch_last=True)
        m.gaussian_conditional.noise_source = SlicedNoise(f"roi_{tag}_gc", 0, 1, 2)
    args = types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3)
    opts = configure_optimizers(imodel, args, max_norm=None) + configure_optimizers(pmodel, args, max_norm=None)
    frames = [f.to(dev) for f in smooth_frames("dp2:gop", 2, 3, 64)]
    qmap = closed_form_input("dp2:qmap", (2, 1, 64, 64), 0.0, 1.0).to(dev)

    class _NoStep:                                       # gradients as they stand right before the optimiser steps
        def __init__(self, o):
            self.o, self.flat, self._sumsq = o, o.flat, o._sumsq

        def zero_grad(self):
            self.o.zero_grad()

        def step(self, *_a, **_k):
            pass

    log = S.roi_gop_step(imodel, pmodel, PixelwiseRateDistortionLoss(), tuple(_NoStep(o) for o in opts), frames, qmap, 1.0)
    # Tolerances: the forward (loss) agrees to fp32 rounding.  Gradients of these 60-layer leaky-ReLU stacks do not quite:
    # a pre-activation within fp32 noise of 0 can land on the other side of the kink when the batch size changes the
    # tile / split-K configuration, and that element's factor (1 vs slope) shifts the (cancelling) gradient sums of the
    # layers below it by up to ~1e-3 -- the same effect, with the same bounds, as the single-process batch-consistency
    # test test_hip_roi.py::test_roi_batch_and_nonsquare_consistency measures between B=2 and 2 x B=1.
    for t, (oc, gn, aux) in enumerate(log):
        l0, l1 = r0["losses"][t], r1["losses"][t]
        assert abs(0.5 * (l0[0] + l1[0]) - float(oc["loss"])) <= 1e-5 * abs(float(oc["loss"])), (t, l0, l1, float(oc["loss"]))
        assert l0[1] == l1[1] and abs(l0[1] - float(gn)) <= 1e-3 * float(gn), (t, l0[1], float(gn))   # clip norm of the GLOBAL running sum
        assert l0[2] == l1[2] and abs(l0[2] - float(aux)) <= 1e-6 * abs(float(aux))
    errs = []
    for key, o in (("grad_i", opts[0]), ("grad_p", opts[2])):
        full = flat_np(o.flat.grad).astype(np.float64)
        for name, p, off in zip(o.flat.names, o.flat.params, o.flat.offsets):
            n = p.numel()
            ref = full[off:off + n]
            scale = float(np.abs(ref).max()) or 1.0
            errs.append((float(np.abs(r0[key][off:off + n] - ref).max()) / scale, f"{key}:{name}"))
    errs.sort(reverse=True)
    p_worst = max(e for e, n in errs if n.startswith("grad_p:"))
    loose = [(e, n) for e, n in errs if e > 1e-3]
    print(f"dp2 gop: {len(errs)} gradient tensors; P model worst |dp - full batch| / max = {p_worst:.2e}; I model worst "
          f"{errs[0][0]:.2e} ({errs[0][1]}), {len(loose)} tensors above 1e-3, median {errs[len(errs) // 2][0]:.1e}")
    assert len(errs) > 500
    assert p_worst <= 1e-4, [e for e in errs if e[1].startswith("grad_p:")][:5]
    # the I model's quality-map feature net holds the known kink element (see above); its effect is amplified here because
    # the frame-0 gradient it is compared against has been clipped from norm ~3000 to 1 before the BPTT terms are added
    assert errs[0][0] < 5e-2 and len(loose) <= 0.05 * len(errs), errs[:8]
    # ... and it sits in one of the kink-bearing conditioning nets of the I model: the quality-feature stacks (leaky ReLU 0.1) or
    # an SFT block's shared MLP (ReLU) -- which of them holds the element within fp32 noise of 0 depends on the kernels' tile /
    # split plans (with the stride-1 layers on the fp16 kernels since round 3 it is ga1_SFT.mlp_shared)
    assert all("qmap_feature_" in n or "_SFT.mlp_" in n for _, n in loose), loose


# ---- RCCL itself, as far as one GPU allows: a world-size-1 "nccl" process group ------------------------------------------
# RCCL refuses two ranks on one device, so the 2-rank tests above exchange through gloo.  These two run ONE rank in a real
# RCCL group (distributed.init_from_env(single=True)): every all-reduce of the reducers is issued to RCCL on the side stream
# with the product's wait_stream ordering, `max_over_ranks` / `any_rank` reduce DEVICE tensors -- and since a one-rank sum is
# the identity, the run must be bit-identical to the same schedule without any process group.
@pytest.mark.dp2("rccl1_train_fused")
def test_rccl_world1_fused_schedule_bit_identical_to_no_process_group(dp2_results, tmp_path):
    import dp_worker
    (r,) = dp2_results("rccl1_train_fused")
    assert str(r["backend"][0]) == "nccl" and int(r["reducer_calls"][0]) == 10 and float(r["max_over_ranks"][0]) == 3.25
    assert not torch.distributed.is_initialized()
    dp_worker.case_train_fused(0, 1, str(tmp_path), tag="local")
    loc = dict(np.load(tmp_path / "local_rank0.npz"))
    assert str(loc["backend"][0]) == "none"
    for k in ("grad_avg", "params", "quantiles", "s1:loss", "s2:loss"):
        np.testing.assert_array_equal(r[k], loc[k], err_msg=k)


@pytest.mark.dp2("rccl1_train_taped")
def test_rccl_world1_taped_executor_bit_identical_to_the_plain_schedule(dp2_results, tmp_path):
    """The native step executor inside a data-parallel run: one rank in a real RCCL group, eight P-frame steps through
    tape.TapedPFrameStep (four of them replayed from the tape, whose Python entries re-issue the reducer's all-reduces on the
    recorded streams), against the same eight steps without a tape and without a process group: bit-identical losses, norms,
    parameters and quantiles; the reducer issued the same number of collectives per step on both routes."""
    import dp_worker
    (r,) = dp2_results("rccl1_train_taped")
    assert str(r["backend"][0]) == "nccl" and int(r["replays"][0]) == 5 and bool(r["taped"][0])
    assert not torch.distributed.is_initialized()
    dp_worker.case_train_taped(0, 1, str(tmp_path), tag="local_taped", taped=False)
    loc = dict(np.load(tmp_path / "local_taped_rank0.npz"))
    assert str(loc["backend"][0]) == "none" and int(r["collectives"][0]) == int(loc["collectives"][0]) > 0
    for k in ["params", "quantiles"] + [f"s{t}:loss" for t in range(1, 9)]:
        np.testing.assert_array_equal(r[k], loc[k], err_msg=k)


@pytest.mark.dp2("rccl1_train_fused")
@pytest.mark.dp2("rccl1_train_fused@0")
@pytest.mark.dp2("rccl1_train_fused@2")
@pytest.mark.dp2("rccl1_train_taped")
@pytest.mark.dp2("rccl1_train_taped@1")
def test_rccl_world1_issue_modes_agree(dp2_results):
    """The reducer's ways of issuing RCCL collectives (STEM_DP_THREADED): 3, the default -- libstem_dp.so: a native helper thread
    with its own communicator enqueues each ncclAllReduce once its producers' events have completed, the compute stream waits for
    a stream flag (distributed._NativeIssuer, include/stem_dp.h); 2 -- the same from a Python thread through torch.distributed
    (_CollectiveIssuer, stem_stream_flag_*); 1 -- that thread, finish() blocking the host; 0 -- round 4's route, asynchronous
    collectives from the reporting stream.  Same schedule, same bits (plain and through the launch tape)."""
    (d,), (m0,), (m2,) = dp2_results("rccl1_train_fused"), dp2_results("rccl1_train_fused@0"), dp2_results("rccl1_train_fused@2")
    assert str(d["issuer"][0]) == "_NativeIssuer" and str(m2["issuer"][0]) == "_CollectiveIssuer" and str(m0["issuer"][0]) == "NoneType"
    assert int(d["reducer_calls"][0]) == int(m0["reducer_calls"][0]) == int(m2["reducer_calls"][0]) == 10
    for k in ("grad_avg", "params", "quantiles", "s1:loss", "s2:loss"):
        np.testing.assert_array_equal(d[k], m0[k], err_msg=k)
        np.testing.assert_array_equal(d[k], m2[k], err_msg=k)
    (t,), (t1,) = dp2_results("rccl1_train_taped"), dp2_results("rccl1_train_taped@1")
    assert int(t1["replays"][0]) == 5 and bool(t1["taped"][0]) and int(t["collectives"][0]) == int(t1["collectives"][0])
    for k in ["params", "quantiles"] + [f"s{i}:loss" for i in range(1, 9)]:
        np.testing.assert_array_equal(t[k], t1[k], err_msg=k)


@pytest.mark.dp2("train_taped")
@pytest.mark.dp2("train_untaped")
def test_two_ranks_taped_executor_bit_identical_to_the_plain_two_rank_run(dp2_results):
    """configs[2] at world size 2 through the native executor: TWO ranks (gloo, sharing cuda:0), eight P-frame steps each through
    tape.TapedPFrameStep -- two ordinary, two recorded, four replayed; the overlapped reducer's all-reduces are re-issued by the
    tape's Python entries in the middle of the replayed backward; the learning rate is halved after step 6, between two replays --
    against the same two ranks on the plain schedule: the replicas stay bit-identical through the replays and equal the untaped
    run's, step by step (losses, clipped norms, auxiliary losses) and in every parameter."""
    t0, t1 = dp2_results("train_taped")
    u0, u1 = dp2_results("train_untaped")
    assert bool(t0["taped"][0]) and bool(t1["taped"][0]) and int(t0["replays"][0]) == int(t1["replays"][0]) == 5
    assert str(t0["backend"][0]) == "gloo" and int(t0["collectives"][0]) == int(u0["collectives"][0]) > 0
    np.testing.assert_array_equal(t0["params"], t1["params"])                # replicas
    np.testing.assert_array_equal(t0["quantiles"], t1["quantiles"])
    for k in range(1, 9):                                                    # the norm of the exchanged gradient is global
        assert t0[f"s{k}:loss"][1] == t1[f"s{k}:loss"][1], k
    for t, u in ((t0, u0), (t1, u1)):                                        # taped == untaped, rank by rank
        for k in ["params", "quantiles"] + [f"s{i}:loss" for i in range(1, 9)]:
            np.testing.assert_array_equal(t[k], u[k], err_msg=k)
    assert not np.array_equal(t0["s1:loss"], t1["s1:loss"])                  # different samples per rank


@pytest.mark.dp2("rccl1_gop")
def test_rccl_world1_gop_accumulator_bit_identical_to_no_process_group(dp2_results, tmp_path):
    import dp_worker
    (r,) = dp2_results("rccl1_gop")
    assert bool(r["active"][0]) and list(r["any_rank"]) == [False, True]
    dp_worker.case_gop(0, 1, str(tmp_path), tag="local_gop")
    loc = dict(np.load(tmp_path / "local_gop_rank0.npz"))
    assert not bool(loc["active"][0])
    # loss / aux values are float64 sums of per-workgroup partials (last bit may differ run to run); clip norms, gradients and
    # parameters come from fixed-order reductions and must be bit-identical
    np.testing.assert_allclose(r["losses"], loc["losses"], rtol=1e-12)
    np.testing.assert_array_equal(r["losses"][:, 1], loc["losses"][:, 1])
    for k in ("params_i", "params_p", "grad_i", "grad_p"):
        np.testing.assert_array_equal(r[k], loc[k], err_msg=k)


# ---- two REAL RCCL ranks: runs wherever two devices are visible, skips on the one-GPU test box -------------------------------------
_TWO = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="two RCCL ranks need a device each (RCCL refuses two ranks on one device)")


@_TWO
@pytest.mark.dp2("rccl2_verify")
def test_rccl_two_devices_equals_full_batch(dp2_results):
    """configs[2] at world size 2 over RCCL/xGMI: one P-frame step (stem/trainSTEM.py:194-218) through the overlapped reducer and
    libstem_dp's own communicator on two devices, against the same step over the global batch computed by rank 0 alone --
    the check `STEM_BENCH_VERIFY=1 bench.py --gpus N` prints as config.data_parallel.loss_vs_single_rank."""
    r0, r1 = dp2_results("rccl2_verify")
    assert int(r0["nranks"][0]) == int(r1["nranks"][0]) == 2 and "libstem_dp" in str(r0["route"][0])
    assert r0["loss_dp"][0] == r1["loss_dp"][0]
    assert 0 <= float(r0["loss_rel"][0]) < 1e-5 and 0 <= float(r0["grad_rel"][0]) < 1e-4, (r0["loss_rel"], r0["grad_rel"])
    assert bool(r0["same"][0]) and bool(r1["same"][0]) and not bool(r0["diff"][0]) and not bool(r1["diff"][0])


@_TWO
@pytest.mark.dp2("rccl2_train_taped")
@pytest.mark.dp2("train_untaped")
def test_rccl_two_devices_taped_equals_the_gloo_pair(dp2_results):
    """Eight P-frame steps on two devices through the launch tape with the native RCCL issue path, against the same two ranks
    sharing one device over gloo on the plain schedule: a two-term sum does not depend on its order, so losses, norms and every
    parameter must be bit-identical, and the replicas identical to each other."""
    t0, t1 = dp2_results("rccl2_train_taped")
    u0, u1 = dp2_results("train_untaped")
    assert str(t0["backend"][0]) == "nccl" and str(t0["issuer"][0]) == "_NativeIssuer" and int(t0["nranks"][0]) == 2
    assert bool(t0["taped"][0]) and bool(t0["replicas_identical"][0]) and bool(t1["replicas_identical"][0])
    np.testing.assert_array_equal(t0["params"], t1["params"])
    for t, u in ((t0, u0), (t1, u1)):
        for k in ["params", "quantiles"] + [f"s{i}:loss" for i in range(1, 9)]:
            np.testing.assert_array_equal(t[k], u[k], err_msg=k)


@pytest.mark.bench_gpus2
def test_bench_gpus2_typed_bare_runs_two_ranks_on_one_device():
    """`python bench.py --gpus 2 --steps 2 --warmup 1 --full` without any launcher (the driver's command form with N = 2): the parent
    starts the two ranks itself before touching the GPU, they share cuda:0 and exchange through gloo (RCCL refuses two ranks on
    one device), and stdout ends with rank 0's ONE JSON line."""
    import json
    import os
    from conftest import DP2, dp2_wait
    assert "bench2" in DP2["jobs"], "bench.py --gpus 2 was not started at collection time"
    (rc,) = dp2_wait("bench2", timeout=900)
    out = open(os.path.join(DP2["dir"], "bench2.out")).read()
    err = open(os.path.join(DP2["dir"], "bench2.err")).read()
    assert rc == 0, f"bench.py --gpus 2 exited with {rc}:\n{err[-3000:]}"
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["config"]["global_batch"] == 32 and rec["config"]["parallelism"] == "dp2"
    assert rec["value"] > 0 and rec["scaling"] == "weak" and "roofline" in rec and "cpu_baseline" not in rec
    # the run's own evidence that it was data parallel: the ranks the exchanging group reports, bit-identical replicas after the
    # timed region, and (STEM_BENCH_VERIFY=1, set by conftest) the first step against rank 0 alone over the global batch
    dp = rec["config"]["data_parallel"]
    assert dp["rccl_nranks"] == 2 and dp["replicas_identical"] is True and "gloo" in dp["exchange_route"]
    lv = dp["loss_vs_single_rank"]
    assert lv["global_batch"] == 32 and lv["rel_diff"] < 1e-5 and lv["averaged_gradient_max_rel_diff"] < 1e-4, lv
