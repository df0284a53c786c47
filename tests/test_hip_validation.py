"""GPU, model level: engine.eval_rate and the validation passes of trainer.py (validate, SeptupletTrainer.validate, validate_pixel,
validate_image) -- against the unfused eval forward (bit for bit), float64 sums of their own likelihoods, explicit per-frame
compositions of existing calls, and the reference's own `validation` (tests/golden/validation.npz, make_golden_validation.py)."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

DEV = torch.device("cuda:0")
CLASSES = ["SpatioTemporalPriorModelWithoutSPMTPM", "SpatioTemporalPriorModelWithoutSPM", "SpatioTemporalPriorModelWithoutTPM",
           "SpatioTemporalPriorModel", "SpatioTemporalPriorModel_Res"]
# (entropy-bottleneck channels, latent channels, batch, latent h, w): 24 -- both chains on the fp32 kernels; 48 -- no multiple of 32
# either; 64 -- the fp16 kernels; 4 x 8 and 8 x 8 latents (the hyper path needs multiples of 4), more than one sample
CONFIGS = [(32, 24, 1, 4, 8), (64, 48, 2, 8, 8), (64, 64, 3, 4, 8)]
PARAMS = [(c, cfg) for c in CLASSES for cfg in CONFIGS] + [("SpatioTemporalPriorModel_Res", (192, 192, 1, 4, 8))]


def rate_bound(*liks):
    """4 * 2^-24 * sum |log2 lik| (tests/test_hip_validation_ops.rate_bound: two float32 ulps of log2f per term, a factor 2 of
    slack) -> (float64 sums of log2 per tensor, bounds per tensor)"""
    l2 = [np.log2(l.detach().cpu().numpy().astype(np.float64)) for l in liks]
    return [float(a.sum()) for a in l2], [4.0 * 2.0 ** -24 * float(np.abs(a).sum()) for a in l2]


@pytest.mark.parametrize("cls,cfg", PARAMS, ids=[f"{c.replace('SpatioTemporalPriorModel', 'STPM')}-c{g[1]}-b{g[2]}-{g[3]}x{g[4]}" for c, g in PARAMS])
def test_eval_rate_equals_the_eval_forward(cls, cfg):
    """engine.eval_rate: y_hat, lik_y, lik_z torch.equal to engine.forward(.., False); loss3 within the derived bound of the float64
    sums of its own likelihoods, loss3[2] == loss3[0] + loss3[1] exactly; the accumulator receives weight * loss3 and the weight;
    no noise offset moves"""
    from spatiotemporalentropymodel_amd import models
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_, closed_form_input
    ebc, cin, B, h, w = cfg
    if getattr(models, cls).HARD_CODED_Z:
        ebc = 256                                        # the two ablations without a spatial prior hard-code 256 hyper-latent channels
    m = closed_form_fill_(getattr(models, cls)(ebc, cin)).to(DEV).eval()
    y_cur = closed_form_input(f"val:{cls}:cur", (B, cin, h, w), -6.0, 6.0).to(DEV)
    y_cond = closed_form_input(f"val:{cls}:cond", (B, cin, h, w), -6.0, 6.0).to(DEV)
    y_cur.view(-1)[::7] = (y_cond.view(-1)[::7] + 2.5) if m.RESIDUAL else 2.5           # rounding ties of the residual / of y itself
    eng = m.engine()
    num_pixels = B * h * w * 256
    offs = (m.entropy_bottleneck._noise_offset, m.gaussian_conditional._noise_offset)
    with torch.no_grad():
        want = eng.forward(y_cur, y_cond, False)[:3]
        acc = torch.zeros(4, dtype=torch.float64, device=DEV)
        acc[3] = 1.5
        got = eng.eval_rate(y_cur, y_cond, num_pixels, acc=acc, weight=float(B))
        again = eng.eval_rate(y_cur, y_cond, num_pixels)
    torch.cuda.synchronize()
    for name, a, b, c in zip(("y_hat", "lik_y", "lik_z"), want, got, again):
        assert a.shape == b.shape and torch.equal(a, b) and torch.equal(b, c), name
    assert (m.entropy_bottleneck._noise_offset, m.gaussian_conditional._noise_offset) == offs
    loss3 = got[3].cpu().numpy()
    assert got[3].dtype == torch.float64 and torch.equal(got[3], again[3])
    assert loss3[2] == loss3[0] + loss3[1]
    (sy, sz), (by, bz) = rate_bound(got[1], got[2])
    print(f"{cls} {cfg}: y_bpp {loss3[0]!r} vs {-sy / num_pixels!r} (bound {by / num_pixels:.3e}), z_bpp {loss3[1]!r} vs {-sz / num_pixels!r} "
          f"(bound {bz / num_pixels:.3e})")
    assert abs(loss3[0] + sy / num_pixels) <= by / num_pixels and abs(loss3[1] + sz / num_pixels) <= bz / num_pixels
    a = acc.cpu().numpy()
    assert a[3] == 1.5 + B and (a[:3] == B * loss3).all()


# ---------------------------------------------------------------------------------------------------------------- validate
def _msh_pair(cls="SpatioTemporalPriorModel_Res"):
    """a deterministic chain: MeanScaleHyperprior's getY rounds in eval mode (no noise), so a sample's losses do not depend on the
    batch it arrives in"""
    from spatiotemporalentropymodel_amd import models
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    imodel = closed_form_fill_(models.MeanScaleHyperprior(64, 96)).to(DEV).train()
    with torch.no_grad():
        imodel.g_a[6].weight.mul_(4.0)
        imodel.g_a[6].bias.mul_(4.0)
    stem = closed_form_fill_(getattr(models, cls)(256 if getattr(models, cls).HARD_CODED_Z else 64, 96)).to(DEV).train()
    return imodel, stem


def _samples(n, nframes, h, w, tag="val"):
    """n samples of nframes frames [3,h,w] -> list over samples of [nframes,3,h,w] device tensors"""
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    return [torch.cat([f[:, :, :h, :w] for f in smooth_frames(f"{tag}:{i}", 1, nframes, 128)]).to(DEV) for i in range(n)]


def _loader(samples, batch):
    """items of `batch` samples (the last one ragged): lists of frame batches [B,3,h,w]"""
    return [[torch.stack([s[t] for s in samples[i:i + batch]]) for t in range(samples[0].shape[0])] for i in range(0, len(samples), batch)]


def _explicit(imodel, stem, loader):
    """stem/trainSTEM.py:265-295 spelled out with existing calls at the loader's batch size -> (sum over P steps of B * loss terms, count)"""
    from spatiotemporalentropymodel_amd.losses import EMLoss
    crit = EMLoss()
    flags = [(mod, mod.training) for m in (imodel, stem) for mod in m.modules()]
    imodel.eval()
    stem.eval()
    tot, cnt = np.zeros(3), 0
    with torch.no_grad():
        for frames in loader:
            _, y_cond = imodel.getY(frames[0])
            for x in frames[1:]:
                y_cur, _ = imodel.getY(x)
                out = stem(y_cur, y_cond)
                y_cond = out["y_hat"]
                oc = crit(out, x)
                B = x.shape[0]
                tot += B * np.array([float(oc["y_bpp_loss"]), float(oc["z_bpp_loss"]), float(oc["loss"])])
                cnt += B
    for mod, flag in flags:
        mod.training = flag
    return tot / cnt, cnt


def test_validate_routes_agree_and_count_samples():
    """validate on both routes against the explicit composition, at loader batch 1, 2 and 3 over 5 samples of 3 frames (ragged last
    items): count = samples x P frames; the fused and the generic route differ only in how fp64 numbers are summed -- both sum the
    (double)log2f terms of the SAME likelihoods (eval_rate's are the eval forward's bits), in another order: n * 2^-53 relative for
    n ~ 1e4 terms, far inside the 1e-6 the two are held to; modes come back as found, no noise offset moves, the scheduler sees the
    returned loss"""
    from spatiotemporalentropymodel_amd import trainer as T
    imodel, stem = _msh_pair()
    imodel.g_s.eval()                                   # a mixed state: restored module by module
    samples = _samples(5, 3, 64, 128)
    seen = []
    sched = types.SimpleNamespace(step=seen.append)
    modes = lambda: [mod.training for m in (imodel, stem) for mod in m.modules()]          # noqa: E731
    offsets = lambda: [mod._noise_offset for m in (imodel, stem) for mod in m.modules() if hasattr(mod, "_noise_offset")]          # noqa: E731
    before, off0 = modes(), offsets()
    ref1 = None
    for batch in (1, 2, 3):
        loader = _loader(samples, batch)
        assert [it[0].shape[0] for it in loader] == {1: [1] * 5, 2: [2, 2, 1], 3: [3, 2]}[batch]
        fused = T.validate(imodel, stem, loader, route="fused", lr_scheduler=sched)
        generic = T.validate(imodel, stem, loader, route="generic", prefetch=False)
        assert modes() == before and offsets() == off0 and stem.training and not imodel.g_s.training
        assert seen[-1] == fused["loss"] and len(seen) == batch
        want, cnt = _explicit(imodel, stem, loader)
        print(f"batch {batch}: fused {fused}, generic {generic}, explicit {want}")
        assert fused["count"] == generic["count"] == cnt == 10.0
        assert all(isinstance(v, float) for v in fused.values()) and set(fused) == {"loss", "y_bpp_loss", "z_bpp_loss", "count"}
        for i, k in enumerate(("y_bpp_loss", "z_bpp_loss", "loss")):
            assert abs(generic[k] - want[i]) <= 1e-12 * abs(want[i]), (k, generic[k], want[i])          # the same fp64 numbers, summed on the device
            assert abs(fused[k] - generic[k]) <= 1e-6 * abs(generic[k]), (k, fused[k], generic[k])
        # the per-sample mean, whatever the batch: a sample's latents do not depend on its batch, its fp16 splits' scales do --
        # inside the project's 1e-4 parity gate
        if ref1 is None:
            ref1 = fused
        assert abs(fused["loss"] - ref1["loss"]) <= 1e-4 * ref1["loss"]
    assert T.validate(imodel, stem, _loader(samples, 2), route="fused", max_items=1)["count"] == 4.0


def test_validate_restores_modes_when_the_loader_raises():
    from spatiotemporalentropymodel_amd import trainer as T
    imodel, stem = _msh_pair("SpatioTemporalPriorModelWithoutSPM")
    stem.HD.eval()
    samples = _samples(2, 2, 64, 64)

    def loader():
        yield _loader(samples, 2)[0]
        raise KeyError("the loader broke")

    before = [mod.training for m in (imodel, stem) for mod in m.modules()]
    for route in ("fused", "generic"):
        with pytest.raises(KeyError, match="the loader broke"):
            T.validate(imodel, stem, loader(), route=route)
        assert [mod.training for m in (imodel, stem) for mod in m.modules()] == before
    with pytest.raises(ValueError, match="route"):
        T.validate(imodel, stem, [], route="taped")
    with pytest.raises(ValueError, match="empty"):
        T.validate(imodel, stem, [], route="fused")


def test_a_model_without_an_engine_validates_on_the_module_route():
    """a (3, 3, 3) bottleneck: route=None and "generic" run the module forward plus EMLoss, "fused" raises the engine's ValueError"""
    from spatiotemporalentropymodel_amd import trainer as T
    from spatiotemporalentropymodel_amd.entropy_models import EntropyBottleneck
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    imodel, stem = _msh_pair("SpatioTemporalPriorModelWithoutSPMTPM")
    stem.entropy_bottleneck = EntropyBottleneck(stem.HE[4].weight.shape[0], filters=(3, 3, 3))
    stem = closed_form_fill_(stem).to(DEV)
    loader = _loader(_samples(2, 2, 64, 64), 2)
    with pytest.raises(ValueError, match="filters"):
        T.validate(imodel, stem, loader, route="fused")
    a, b = T.validate(imodel, stem, loader), T.validate(imodel, stem, loader, route="generic")
    want, cnt = _explicit(imodel, stem, loader)
    # the module route's log-sum adds its workgroups' fp64 partials with atomics, in whatever order they arrive: two runs agree to the
    # rounding of an fp64 sum of a few terms, not to the bit (the fused route's fixed-order partials do)
    assert set(a) == set(b) and all(abs(a[k] - b[k]) <= 1e-12 * abs(b[k]) for k in a), (a, b)
    assert a["count"] == cnt == 2.0 and abs(a["loss"] - want[2]) <= 1e-12 * want[2]
    assert np.isfinite(a["loss"]) and a["loss"] > 0


# ---------------------------------------------------------------------------------------------------------------- no disturbance
def _train_state(route, validate, monkeypatch):
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd import selfcheck as S
    from spatiotemporalentropymodel_amd import trainer as T
    from spatiotemporalentropymodel_amd.optim import configure_optimizers
    for k in T.SCHEDULE_DEFAULTS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(F, "_STREAM_PRIO", None)
    torch.manual_seed(11)
    imodel, stem = S.build_models(64, 96, 64, 96, DEV, closed_form=False, inject_noise=False)       # Philox noise: the offsets matter
    stem.train()
    opt, aux = configure_optimizers(stem, types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3))
    g = torch.Generator(device=DEV).manual_seed(3)
    sept = [[torch.rand(2, 3, 128, 128, device=DEV, generator=g) for _ in range(7)] for _ in range(2)]
    test_loader = [[torch.rand(2, 3, 64, 64, device=DEV, generator=g) for _ in range(3)] for _ in range(2)]
    tr = T.SeptupletTrainer(imodel, stem, opt, aux, route=route)
    sched = T.tuned_schedule(DEV)
    res = None
    with sched:
        log = tr.train_septuplet(sept[0], rand=1.0, next_images=sept[1])            # the prefetcher holds the next item's first latents
        if validate:
            res = tr.validate(test_loader, route="fused")
            res2 = tr.validate(test_loader, route="generic")
            assert abs(res["loss"] - res2["loss"]) <= 1e-6 * res2["loss"] and res["count"] == 8.0
        log += tr.train_septuplet(sept[1], rand=1.0)
        tr.finish()
    torch.cuda.synchronize()
    if route == "taped":
        assert tr.step_fn.taped and tr.step_fn.replays == 9            # steps 5, 6 and the second item's six were replays
    losses = [float(oc["loss"]) for oc, _, _ in log]
    offsets = [mod._noise_offset for m in (imodel, stem) for mod in m.modules() if hasattr(mod, "_noise_offset")]
    state = [opt.flat.data.clone(), aux.flat.data.clone(), opt.m.clone(), opt.v.clone(), aux.m.clone(), aux.v.clone()]
    return state, (opt.t, aux.t, offsets, [mod.training for m in (imodel, stem) for mod in m.modules()]), losses, res


@pytest.mark.parametrize("route", ["fused", "taped"])
def test_validation_does_not_disturb_training(route, monkeypatch):
    """two train_septuplet calls (12 P-frame steps) with validate() on both routes between them against the same two calls without:
    every parameter, both optimiser states, the step counts, the noise offsets of both models and the module modes bit-identical,
    and so every loss of the second call.  taped: the pass runs between two replays of the recorded tape."""
    a_state, a_meta, a_losses, _ = _train_state(route, False, monkeypatch)
    b_state, b_meta, b_losses, res = _train_state(route, True, monkeypatch)
    assert res is not None and np.isfinite(res["loss"]) and res["loss"] > 0
    assert a_losses == b_losses, (a_losses, b_losses)
    assert a_meta == b_meta
    for i, (x, y) in enumerate(zip(a_state, b_state)):
        assert torch.equal(x, y), i


# ---------------------------------------------------------------------------------------------------------------- pixel / image
def test_validate_pixel_and_validate_image_equal_their_compositions():
    """validate_pixel with one loader (_validation_stem_baseline) and with a list of (frames, Qmap) loaders (_validation_stem_roi), and
    validate_image (test_epoch), at 64 x 64 frames against the loops of the reference spelled out with the same forwards and criteria"""
    from spatiotemporalentropymodel_amd import models
    from spatiotemporalentropymodel_amd import trainer as T
    from spatiotemporalentropymodel_amd.layers import to_nchw
    from spatiotemporalentropymodel_amd.losses import PixelwiseRateDistortionLoss, RateDistortionLoss, quality2lambda
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_scaled_
    items = [[s[t:t + 1] for t in range(3)] for s in _samples(2, 3, 64, 64, "pix")]
    rd = RateDistortionLoss(lmbda=1e-2)
    close = lambda a, b: abs(a - b) <= 1e-12 * abs(b)          # noqa: E731  (the same fp64 device numbers, summed on the device / on the host)

    def nchw(out):                                      # an image model of the zoo returns x_hat in NHWC memory: the layout kernel, as image_step
        return dict(out, x_hat=to_nchw(out["x_hat"])) if not out["x_hat"].is_contiguous() else out

    # baseline: every frame counts, the I frame included
    mi = closed_form_fill_scaled_(models.MeanScaleHyperprior(64, 96), "msh", 1.0).to(DEV).train()
    mp = closed_form_fill_scaled_(models.stem_baseline(), "base_p", 0.7).to(DEV).train()
    got = T.validate_pixel(mi, mp, items, rd)
    assert mi.training and mp.training and set(got) == {"loss", "mse_loss", "bpp_loss"}
    mi.eval(), mp.eval()
    tot, cnt = {k: 0.0 for k in got}, 0
    with torch.no_grad():
        for frames in items:
            for idx, x in enumerate(frames):
                out = nchw(mi(x) if idx == 0 else mp(x, x_cond))          # noqa: F821
                x_cond = out["x_hat"]
                oc = rd(out, x)
                for k in tot:
                    tot[k] += float(oc[k])
                cnt += 1
    assert cnt == 6 and all(close(got[k], tot[k] / cnt) for k in got), (got, tot)

    # image model: test_epoch
    mi.train()
    img = T.validate_image(mi, [f for frames in items for f in frames[:2]], rd)
    assert mi.training and set(img) == {"loss", "bpp_loss", "mse_loss", "aux_loss"}
    mi.eval()
    tot = {k: 0.0 for k in img}
    with torch.no_grad():
        for x in [f for frames in items for f in frames[:2]]:
            oc = rd(nchw(mi(x)), x)
            for k in ("loss", "bpp_loss", "mse_loss"):
                tot[k] += float(oc[k])
            tot["aux_loss"] += float(mi.aux_loss())
    assert all(close(img[k], tot[k] / 4) for k in img), (img, tot)

    # variable rate: one loader per quality level
    ri = closed_form_fill_scaled_(models.stem_roi_i(), "roi_i", 0.7).to(DEV).train()
    rp = closed_form_fill_scaled_(models.stem_roi(), "roi_p", 0.7).to(DEV).train()
    crit = PixelwiseRateDistortionLoss()
    loaders = [[(frames, torch.full((1, 1, 64, 64), q, device=DEV)) for frames in items[:1 + i]] for i, q in enumerate((0.2, 0.8))]
    res = T.validate_pixel(ri, rp, loaders, crit)
    assert isinstance(res, list) and len(res) == 2 and ri.training and rp.training
    ri.eval(), rp.eval()
    for got, loader in zip(res, loaders):
        assert set(got) == {"loss", "mse_loss", "bpp_loss", "mse"}
        tot, cnt = {k: 0.0 for k in got}, 0
        with torch.no_grad():
            for frames, qmap in loader:
                lm = quality2lambda(qmap)
                for idx, x in enumerate(frames):
                    out = nchw(ri(x, qmap) if idx == 0 else rp(x, x_cond, qmap))
                    x_cond = out["x_hat"]
                    oc = crit(out, x, lm)
                    for k in ("loss", "mse_loss", "bpp_loss"):
                        tot[k] += float(oc[k])
                    tot["mse"] += float(RateDistortionLoss()(out, x)["mse_loss"])
                    cnt += 1
        assert cnt == 3 * len(loader) and all(close(got[k], tot[k] / cnt) for k in got), (got, tot)
    assert res[0]["loss"] != res[1]["loss"]


# ---------------------------------------------------------------------------------------------------------------- the reference
class _ItemNoise:
    """noise_source of the I-frame model's GaussianConditional that repeats what make_golden_validation.py fed the reference: getY
    call `frame` of loader item `item` (batch 1 there) drew closed_form_input("noise:iframe_gc:<item * nframes + frame>").  Here a
    loader item holds `batch` of those items: sample i of call c gets draw (first item + i) * nframes + c % nframes."""

    def __init__(self, nframes, batch):
        self.nframes, self.batch, self.calls = nframes, batch, 0

    def __call__(self, shape, device):
        from spatiotemporalentropymodel_amd.weights import closed_form_input
        item0, frame = (self.calls // self.nframes) * self.batch, self.calls % self.nframes
        self.calls += 1
        one = (1,) + tuple(shape[1:])
        return torch.cat([closed_form_input(f"noise:iframe_gc:{(item0 + i) * self.nframes + frame}", one, -0.5, 0.5) for i in range(shape[0])]).to(device)


@pytest.mark.parametrize("route", ["fused", "generic"])
@pytest.mark.parametrize("batch", [1, 3])
def test_validate_against_the_references_validation(route, batch):
    """trainer.validate on the models, frames and noise of tests/golden/validation.npz against the loss the reference's own
    `validation` (stem/trainSTEM.py:265-295) returned in float64: 1e-4 relative, the project's parity gate (the reference's own
    float32 run lies within a third of it: rel32 in the fixture), at loader batch 1 -- the reference's -- and with the three items
    as ONE batch of 3.  Two calls on a ReduceLROnPlateau(patience=0) scheduler: the learning rates after each equal the reference's."""
    from spatiotemporalentropymodel_amd import models
    from spatiotemporalentropymodel_amd import trainer as T
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    g = np.load(os.path.join(GOLDEN, "validation.npz"))
    items, nframes, h, w = (int(v) for v in g["cfg"])
    assert float(g["rel32"][0]) <= 1e-4 / 3 and g["loss64"][0] == g["loss64"][1]
    # tests/golden/make_golden.py:eval_gop_models restated (as tests/test_hip_codec.py does): the small I-frame model with its last
    # analysis layer x 4 / first synthesis layer x 1/4, the small SpatioTemporalPriorModel_Res, closed-form weights
    imodel = closed_form_fill_(models.JointAutoregressiveHierarchicalPriors(64, 96))
    with torch.no_grad():
        imodel.g_a[6].weight.mul_(4.0)
        imodel.g_a[6].bias.mul_(4.0)
        imodel.g_s[0].weight.mul_(0.25)
    stem = closed_form_fill_(models.SpatioTemporalPriorModel_Res(64, 96))
    imodel, stem = imodel.to(DEV).train(), stem.to(DEV).train()
    samples = [torch.from_numpy(g[f"frames:{i}"]).to(DEV) for i in range(items)]
    assert samples[0].shape == (nframes, 3, h, w)
    loader = _loader(samples, batch)
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(dummy, "min", patience=0, factor=0.2)
    want = float(g["loss64"][0])
    for call in range(2):
        imodel.gaussian_conditional.noise_source = _ItemNoise(nframes, batch)          # every call starts at draw 0, as the fixture's
        res = T.validate(imodel, stem, loader, route=route, lr_scheduler=sched)
        print(f"{route} batch {batch} call {call}: loss {res['loss']!r}, reference float64 {want!r}, rel {abs(res['loss'] - want) / want:.3e} "
              f"(reference float32: {float(g['rel32'][0]):.3e}; tie margin {float(g['tie_margin'][0]):.3e})")
        assert res["count"] == items * (nframes - 1)
        assert abs(res["loss"] - want) <= 1e-4 * want
        assert dummy.param_groups[0]["lr"] == float(g["lr"][call])
    assert imodel.training and stem.training
