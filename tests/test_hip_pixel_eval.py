"""GPU: the evaluation loop of the pixel-domain models and MeanScaleHyperprior against the reference's own evaluation functions
(tests/golden/pixel_eval_roi.npz, pixel_eval_baseline.npz: tests/golden/make_golden_pixel_eval.py runs inference_i / inference_p of
stem_roi/eval_stem_roi.py and eval_stem_baseline.py), and the one-shot coding path under every model that has one against the route
spelled from the entropy models' public primitives."""
import math

import numpy as np
import pytest
import torch

import pixel_eval_fixture as fx
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.detach().cpu().contiguous().numpy()


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available()
    return functional


@pytest.fixture(scope="module")
def E():
    from spatiotemporalentropymodel_amd import evaluation
    return evaluation


@pytest.fixture(scope="module")
def chains(golden):
    """name -> (fixture, model_i, model_p, quality map or None), built once"""
    groi, gbase = golden("pixel_eval_roi.npz"), golden("pixel_eval_baseline.npz")
    return {"roi": (groi, *fx.roi_chain(DEV, groi), torch.from_numpy(groi["qmap"]).to(DEV)),
            "baseline": (gbase, *fx.baseline_chain(DEV, gbase), None)}


@pytest.fixture(scope="module")
def frames():
    return [f.to(DEV) for f in fx.frames3()]


# ----------------------------------------------------------------------------- 1. strings
def _coded_from_primitives(em, values, indexes, means):
    """EntropyModel.compress as it was spelled before the coding kernels: quantize(..., "symbols"), the indexes as a tensor, both
    transposed to the reference's flattening order on the host, the host coder once per batch element"""
    from spatiotemporalentropymodel_amd.entropy_models import RansEncoder
    sym = em.quantize(values, "symbols", means).cpu().contiguous().numpy()
    idx = indexes.int().cpu().contiguous().numpy()
    assert sym.shape == idx.shape == tuple(values.shape)
    return sym, [RansEncoder().encode_with_indexes(sym[i], idx[i], em.host_tables()) for i in range(sym.shape[0])]


def _pixel_case(cls, tag, size):
    from spatiotemporalentropymodel_amd.weights import closed_form_input, smooth_frames
    m = fx.build(cls, tag, fx.ROI_CONV_SCALE, DEV)
    x, xc = (f.to(DEV) for f in smooth_frames("pixeleval:" + tag, 1, 2, size))
    q = closed_form_input("pixeleval:q:" + tag, (1, 1, size, size), 0.0, 1.0).to(DEV)
    args = [x] + ([xc] if m.TEMPORAL else []) + ([q] if m.QMAP else [])
    y, y_cond, z = m._latents(*m._split_args(args))
    return m, args, ([xc] if m.TEMPORAL else []), y, z, lambda z_hat: m._gaussian_params(z_hat, y_cond).chunk(2, 1)


def _case(name):
    from spatiotemporalentropymodel_amd import codec, functional as Fn, models
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_, closed_form_input, smooth_frames
    if name == "stem_roi_i":
        return _pixel_case(models.stem_roi_i, "roi_i", 128)
    if name == "stem_roi":
        return _pixel_case(models.stem_roi, "roi_p", 128)
    if name == "stem_baseline":
        return _pixel_case(models.stem_baseline, "base_p", 64)
    if name == "MeanScaleHyperprior":
        m = fx.build(models.MeanScaleHyperprior, "msh", 1.0, DEV, None, 64, 96)
        x = smooth_frames("pixeleval:msh", 1, 1, 64)[0].to(DEV)
        y = m.g_a(x)
        return m, [x], [], y, m.h_a(y), m._gaussian_params
    # a latent-domain STEM model without a spatial prior (temporal + hyper prior): codec.stem_compress's one-shot branch
    m = closed_form_fill_(models.SpatioTemporalPriorModelWithoutSPM(256, 96)).to(DEV).eval()      # (the SPM-less ablations hard-code 256 hyper channels)
    m.update(force=True)
    y = Fn.to_nhwc(closed_form_input("pixeleval:stem:y", (1, 96, 8, 8), -6, 6).to(DEV))
    y_cond = Fn.to_nhwc(closed_form_input("pixeleval:stem:c", (1, 96, 8, 8), -6, 6).to(DEV))
    eng = m.engine()
    he_in = Fn.empty_nhwc(1, 192, 8, 8, DEV)
    Fn.copy_channels(y, he_in[:, :96]), Fn.copy_channels(y_cond, he_in[:, 96:])
    z = codec._chain(eng.HE, he_in)

    def params(z_hat):
        return codec._one_shot(m, codec._chain(eng.HD, Fn.to_nhwc(z_hat)), codec._chain(eng.TPM, y_cond))

    return m, [y, y_cond], [y_cond], y, z, params


@pytest.mark.parametrize("name", ["stem_roi_i", "stem_roi", "stem_baseline", "MeanScaleHyperprior", "SpatioTemporalPriorModelWithoutSPM"])
def test_strings_equal_the_route_of_primitives(name):
    with torch.no_grad():
        m, args, cond, y, z, params = _case(name)
        eb, gc = m.entropy_bottleneck, m.gaussian_conditional
        enc = m.compress(*args)
        medians = eb._get_medians().detach().expand(z.size(0), -1, 1, 1)
        z_sym, z_strings = _coded_from_primitives(eb, z, eb._build_indexes(z.size()).to(DEV), medians)
        assert enc["strings"][1] == z_strings, f"{name}: z string differs from the primitives route"
        assert tuple(enc["shape"]) == tuple(z.shape[-2:])
        z_hat = eb.dequantize(torch.from_numpy(z_sym).to(DEV), medians)
        scales, means = params(z_hat)
        y_sym, y_strings = _coded_from_primitives(gc, y, gc.build_indexes(scales), means)
        assert enc["strings"][0] == y_strings, f"{name}: y string differs from the primitives route"
        assert np.abs(y_sym).max() > 0 and len(y_strings[0]) > 16                      # the strings carry symbols
        # the decoder lands on symbol + mean of the primitives route, bit for bit, and so does the bottleneck's own round trip
        dec = m.decompress(enc["strings"], enc["shape"], *cond)
        y_hat = dec["y_hat"] if isinstance(dec, dict) else dec
        want = gc.dequantize(torch.from_numpy(y_sym).to(DEV), means)
        np.testing.assert_array_equal(host(y_hat).view(np.int32), host(want).view(np.int32))
        np.testing.assert_array_equal(host(eb.decompress(enc["strings"][1], enc["shape"])).view(np.int32), host(z_hat).view(np.int32))
        # the public signature with a tensor of indexes still codes the same string
        assert gc.compress(y, gc.build_indexes(scales), means=means) == y_strings
        again = gc.decompress(y_strings, gc.build_indexes(scales), means=means)
        np.testing.assert_array_equal(host(again).view(np.int32), host(y_hat).view(np.int32))


@pytest.mark.parametrize("name", ["stem_roi_i", "stem_roi", "stem_baseline", "MeanScaleHyperprior", "SpatioTemporalPriorModelWithoutSPM"])
def test_decompress_reproduces_the_eval_forward(name):
    """decompress(compress(x))["y_hat"] equals model(x)["y_hat"] in eval mode, bit for bit.

    The pixel-domain / image models run the same layer calls in forward and in the coding calls.  A latent-domain STEM model's forward
    is the fused engine's schedule, whose convolution epilogues hand fp16 planes to the next layer (scaled by a bound of |output|),
    where codec._chain splits every layer's fp32 input by its measured maximum: the means then differ in their last bits (3.8e-6 at
    |y_hat| 6.5, never a symbol).  The eval forward of a model without a spatial prior returns round(y - means) + means, so it runs
    codec._chain's arithmetic (StemEngine._forward, `ep`); the training forward and the strings are what they were."""
    with torch.no_grad():
        m, args, cond, y, z, params = _case(name)
        enc = m.compress(*args)
        dec = m.decompress(enc["strings"], enc["shape"], *cond)
        y_hat = host(dec["y_hat"] if isinstance(dec, dict) else dec)
        fwd = host(m(*args)["y_hat"])
    differ = y_hat.view(np.int32) != fwd.view(np.int32)
    assert not differ.any(), (f"{name}: {int(differ.sum())} of {differ.size} latents differ from the eval forward, max |difference| "
                              f"{float(np.abs(y_hat - fwd).max()):.3e} at max |y_hat| {float(np.abs(fwd).max()):.3e}, "
                              f"{int((np.rint(y_hat - fwd) != 0).sum())} by a whole symbol")


# ----------------------------------------------------------------------------- 2. MeanScaleHyperprior
def test_mean_scale_hyperprior_matches_reference(golden):
    from spatiotemporalentropymodel_amd import zoo
    from spatiotemporalentropymodel_amd.models import MeanScaleHyperprior
    from spatiotemporalentropymodel_amd.selfcheck import NoiseFeed
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_scaled_
    g = golden("pixel_eval_baseline.npz")
    m = closed_form_fill_scaled_(MeanScaleHyperprior(64, 96), "msh", 1.0).to(DEV).train()
    keys = [f"{k}|{','.join(map(str, v.shape))}" for k, v in m.state_dict().items()]
    assert keys == list(g["keys:MeanScaleHyperprior"])
    m.entropy_bottleneck.noise_source = NoiseFeed("msh_eb")
    m.gaussian_conditional.noise_source = NoiseFeed("msh_gc")
    out = m(torch.from_numpy(g["train:x"]).to(DEV))
    assert set(out) == {"y", "y_hat", "x_hat", "likelihoods"}
    assert_close(host(out["y"]), g["train:y"], what="y", floor=0.1)
    assert_close(host(out["y_hat"]), g["train:y_hat"], what="y_hat", floor=0.1)
    assert_close(host(out["x_hat"]), g["train:x_hat"], what="x_hat", floor=0.1)
    assert_close(host(out["likelihoods"]["y"]), g["train:lik_y"], atol=1e-9, what="lik_y", floor=0.1)
    assert_close(host(out["likelihoods"]["z"]), g["train:lik_z"], atol=1e-9, what="lik_z", floor=0.1)
    # getY rounds in eval mode (mbt2018's adds noise there too)
    m.eval()
    y, yq = m.getY(torch.from_numpy(g["train:x"]).to(DEV))
    np.testing.assert_array_equal(host(yq), np.rint(host(y)))
    small, large = zoo.models["mbt2018-mean"](quality=4), zoo.models["mbt2018-mean"](quality=5)
    assert isinstance(small, MeanScaleHyperprior) and (small.N, small.M, large.N, large.M) == (128, 192, 192, 320)
    assert tuple(small.g_a[6].weight.shape[:2]) == (192, 128) and tuple(small.h_s[4].weight.shape[:2]) == (384, 288)
    with pytest.raises(RuntimeError):
        zoo.models["mbt2018-mean"](quality=4, pretrained=True)
    with pytest.raises(ValueError):
        zoo.models["mbt2018-mean"](quality=9)


# ----------------------------------------------------------------------------- 3. the reference, frame by frame
@pytest.mark.parametrize("chain", ["roi", "baseline"])
def test_frames_match_the_reference(E, chains, frames, chain):
    """Every frame through inference_pixel_i / inference_pixel_p, each P frame conditioned on the REFERENCE's recorded previous x_hat
    (a one-shot string depends on fp32 rounding decisions, so a flip must not compound).  Gates, those of
    tests/test_hip_roi.py::test_roi_codec_roundtrip_and_rate: string lengths within max(1 %, 4 bytes), mean |x_hat - ref| < 2e-3,
    x_hat in [0, 1], `shape` equal; estimate_bpp within 2e-3 relative."""
    g, model_i, model_p, qmap = chains[chain]
    report, failed = [], []
    for t, x in enumerate(frames):
        if t == 0:
            out = E.inference_pixel_i(model_i, x, qmap, with_msssim=False)
        else:
            out = E.inference_pixel_p(model_p, x, torch.from_numpy(g[f"f{t - 1}:x_hat"]).to(DEV), qmap, with_msssim=False)
        nb = np.array([len(out["strings"][0][0]), len(out["strings"][1][0])])
        ref_nb = g[f"f{t}:nbytes"]
        ref_bpp, ref_est, ref_psnr = g[f"f{t}:scalars"]
        dist = float((out["x_hat"] - torch.from_numpy(g[f"f{t}:x_hat"]).to(DEV)).abs().mean())
        est = abs(out["estimate_bpp"] - ref_est) / abs(ref_est)
        report.append(f"frame {t}: bytes {nb.tolist()} vs {ref_nb.tolist()}, mean |x_hat - ref| {dist:.3e}, estimate_bpp {out['estimate_bpp']:.6f} "
                      f"vs {ref_est:.6f} ({est:.2e} relative), psnr {out['psnr']:.4f} vs {ref_psnr:.4f}")
        ok = (np.all(np.abs(nb - ref_nb) <= np.maximum(0.01 * ref_nb, 4)) and dist < 2e-3 and est <= 2e-3
              and float(out["x_hat"].min()) >= 0 and float(out["x_hat"].max()) <= 1 and out["shape"] == tuple(g[f"f{t}:shape"])
              and tuple(out["x_hat"].shape) == (1, 3, *fx.SIZE) and out["bits"] == 8.0 * nb.sum()
              and out["bpp"] == 8.0 * nb.sum() / (fx.SIZE[0] * fx.SIZE[1]) and out["ms-ssim"] is None
              and abs(out["y_bpp"] + out["z_bpp"] - out["bpp"]) < 1e-12 and abs(out["estimate_y_bpp"] + out["estimate_z_bpp"] - out["estimate_bpp"]) < 1e-9
              and (("psnr_roi" in out) == (qmap is not None)))
        if not ok:
            failed.append(t)
    print("\n".join([f"[{chain}]"] + report))
    assert not failed, f"{chain}: frames {failed} miss a gate\n" + "\n".join(report)


# ----------------------------------------------------------------------------- 4. the chain
@pytest.mark.parametrize("chain", ["roi", "baseline"])
def test_eval_gop_pixel_is_the_two_functions_with_the_cropped_feedback(E, chains, frames, chain):
    g, model_i, model_p, qmap = chains[chain]
    res = E.eval_gop_pixel(model_i, model_p, frames, qmaps=qmap, gop=12, with_msssim=False)
    assert [f["type"] for f in res["frames"]] == ["I", "P", "P"]
    by_hand, x_cond = [], None
    for t, x in enumerate(frames):
        out = E.inference_pixel_i(model_i, x, qmap, with_msssim=False) if t == 0 else E.inference_pixel_p(model_p, x, x_cond, qmap, with_msssim=False)
        x_cond = out["x_hat"]
        by_hand.append(out)
    for a, b in zip(res["frames"], by_hand):
        assert a["strings"] == b["strings"] and a["shape"] == b["shape"]
        assert torch.equal(a["x_hat"].view(torch.int32), b["x_hat"].view(torch.int32))
        for k in ("psnr", "bpp", "bits", "estimate_bpp"):
            assert a[k] == b[k], k
        if qmap is not None:      # the weighted sum adds its workgroups' float64 partials in arrival order: equal to ~1024 * 2^-53 relative
            assert abs(a["psnr_roi"] - b["psnr_roi"]) <= 1e-11
    for key, ave in (("psnr", "psnr_ave"), ("bpp", "bpp_ave"), ("bits", "bits_ave"), ("estimate_bpp", "estimate_bpp_ave")):
        assert abs(res[ave] - sum(f[key] for f in by_hand) / 3) <= 1e-12 * abs(res[ave]), ave
    if qmap is not None:
        assert abs(res["psnr_roi_ave"] - sum(f["psnr_roi"] for f in res["frames"]) / 3) <= 1e-12 * abs(res["psnr_roi_ave"])
    else:
        assert res["psnr_roi_ave"] is None
    assert res["msssim_ave"] is None


# ----------------------------------------------------------------------------- 5. psnr_roi
def test_psnr_roi_against_float64(E, F, golden, frames):
    """sum w (x - x_hat)^2 by the HIP reduction against float64 numpy, 1e-6 relative: the kernel's term lam * (d * d) with d = xhat - x
    carries four fp32 roundings (one subtraction, two products, and d enters the square twice: (1 + e)^2 (1 + e')(1 + e''), at most
    4 * 2^-24 = 2.4e-7); every term is non-negative, so the bound carries to the sum, which is accumulated in float64."""
    g = golden("pixel_eval_roi.npz")
    h, w = fx.SIZE
    x = frames[0].unsqueeze(0)
    x_hat = torch.from_numpy(g["f0:x_hat"]).to(DEV)
    mask = torch.zeros(1, 1, h, w)
    mask[..., 20:70, 10:50] = 1.0
    for name, wmap in (("mask", mask), ("gradient", E.quality_map("horizontal", h, w)), ("uniform", E.quality_map("uniform", h, w, 31))):
        wd = wmap.to(DEV)
        want = float((wmap.double().numpy() * (host(x_hat).astype(np.float64) - host(x).astype(np.float64)) ** 2).sum())
        got = float(F.weighted_sqerr_sum(x_hat.contiguous(), x.contiguous(), wd.contiguous()))
        assert abs(got - want) <= 1e-6 * want, (name, got, want)
        ref = -10 * math.log10(want / (3 * float(wmap.double().sum())))
        val = E.psnr_roi(x, x_hat, wd)
        assert abs(val - ref) <= 10 / math.log(10) * 1.1e-6, (name, val, ref)
    assert E.psnr_roi(x, x_hat, torch.zeros(1, 1, h, w, device=DEV)) is None
    assert E.psnr_roi(x, x_hat, mask.to(DEV)) != E.psnr_roi(x, x_hat, torch.ones(1, 1, h, w, device=DEV))
    uniform = E.psnr_roi(x, x_hat, torch.ones(1, 1, h, w, device=DEV))
    assert abs(uniform - E.psnr(x, x_hat)) < 1e-4                                   # a unit weight is the plain PSNR
