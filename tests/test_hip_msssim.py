"""GPU: stem_ms_ssim (csrc/msssim.hip) through functional.ms_ssim, evaluation.ms_ssim_device and eval_gop(with_msssim="device").

Yardstick: the float64 evaluation of the algorithm evaluation.ms_ssim defines (its body with .double() and the same fp32-rounded
window), computed here with torch-CPU operators.  The host fp32 function's own distance from float64 on the same cases is the
scale of the bounds: the device result must be within 4 x the LARGEST host-fp32 error of the whole case table of this run (the
table maximum, not the per-case value: the order of the two separable passes alone moves single cases by a factor of 7 and the
maximum by 2), and never beyond the project's 1e-4 relative.  Every run prints device, host fp32 and float64 side by side.
"""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import f64_gate

pytestmark = pytest.mark.gpu

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SIZES = [(1, 3, 161, 161), (2, 3, 177, 211), (1, 3, 256, 256), (1, 3, 1080, 1920), (3, 1, 192, 320)]
DISTORTIONS = ["noise .01", "noise .05", "blur", "quant 5 bit", "identical", "flat vs flat+eps"]


def _filter(x, k):
    C = x.shape[1]
    x = torch.nn.functional.conv2d(x, k.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return torch.nn.functional.conv2d(x, k.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)


def ms_ssim_terms(x, y, data_range, dtype):
    """the body of evaluation.ms_ssim in `dtype`, window rounded to fp32 first -> (per image [B], clamped per-scale means [B,C,5])"""
    from spatiotemporalentropymodel_amd.evaluation import _gauss_window
    x, y = x.to(dtype), y.to(dtype)
    k = _gauss_window().to(dtype)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    terms = []
    for level in range(5):
        mu1, mu2 = _filter(x, k), _filter(y, k)
        s11 = _filter(x * x, k) - mu1 * mu1
        s22 = _filter(y * y, k) - mu2 * mu2
        s12 = _filter(x * y, k) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
        ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
        if level < 4:
            terms.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = [s % 2 for s in x.shape[2:]]
            x = torch.nn.functional.avg_pool2d(x, kernel_size=2, padding=pad)
            y = torch.nn.functional.avg_pool2d(y, kernel_size=2, padding=pad)
        else:
            terms.append(torch.relu(ssim_map.flatten(2).mean(-1)))
    t = torch.stack(terms)                                            # [5,B,C]
    w = torch.tensor(WEIGHTS, dtype=dtype).view(-1, 1, 1)
    return torch.prod(t ** w, dim=0).mean(1).double().numpy(), t.permute(1, 2, 0).double().numpy()


@functools.lru_cache(maxsize=None)
def natural(B, C, H, W, seed):
    """smooth, natural-like images: sums of bilinearly upsampled noise at strides 64 / 16 / 4 / 1, normalised to [0,1]"""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, C, H, W)
    for s in (64, 16, 4, 1):
        n = torch.rand(B, C, -(-H // s) + 1, -(-W // s) + 1, generator=g)
        x += torch.nn.functional.interpolate(n, scale_factor=s, mode="bilinear", align_corners=False)[:, :, :H, :W] * (s ** 0.5)
    return (x - x.amin()) / (x.amax() - x.amin())


def distorted(x, name, g):
    if name == "noise .01":
        return x, (x + 0.01 * torch.randn(x.shape, generator=g)).clamp(0, 1)
    if name == "noise .05":
        return x, (x + 0.05 * torch.randn(x.shape, generator=g)).clamp(0, 1)
    if name == "blur":
        return x, torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), 3, 1)
    if name == "quant 5 bit":
        return x, torch.round(x * 31) / 31
    if name == "identical":
        return x, x.clone()
    assert name == "flat vs flat+eps"
    flat = torch.full_like(x, 0.5)
    return flat, flat + 1e-3 * torch.randn(x.shape, generator=g)


def device_run(x, y, data_range=1.0):
    from spatiotemporalentropymodel_amd import functional as F
    dev = torch.device("cuda:0")
    ms, mse, terms = F.ms_ssim(x.to(dev), y.to(dev), data_range, return_terms=True)
    return ms, mse, terms


@functools.lru_cache(maxsize=None)
def table():
    """every case once: inputs, float64, host fp32 (evaluation.ms_ssim itself for the value, its body in fp32 for the terms), device"""
    from spatiotemporalentropymodel_amd import evaluation
    cases = []
    todo = [(shape, name, 1.0) for shape in SIZES for name in DISTORTIONS] + [((1, 3, 256, 256), "noise .01", 255.0)]
    for shape, name, data_range in todo:
        base = natural(*shape, seed=1)
        x, y = distorted(base, name, torch.Generator().manual_seed(7))
        x, y = (x * data_range).contiguous(), (y * data_range).contiguous()
        exact, exact_terms = ms_ssim_terms(x, y, data_range, torch.float64)
        host32 = evaluation.ms_ssim(x, y, data_range=data_range)
        _, host32_terms = ms_ssim_terms(x, y, data_range, torch.float32)
        ms, mse, terms = device_run(x, y, data_range)
        cases.append({"what": f"{'x'.join(map(str, shape))} {name} range {data_range:g}", "x": x, "y": y, "data_range": data_range,
                      "exact": exact, "exact_terms": exact_terms, "host_err": abs(host32 - float(exact.mean())),
                      "host_terms_err": float(np.abs(host32_terms - exact_terms).max()),
                      "exact_mse": ((x.double() - y.double()) ** 2).flatten(1).mean(1).numpy(),
                      "ms": ms.double().cpu().numpy(), "mse": mse.double().cpu().numpy(), "terms": terms.double().cpu().numpy()})
    return cases


def test_every_case_is_in_the_table():
    assert len(table()) == len(SIZES) * len(DISTORTIONS) + 1
    assert all(np.isfinite(c["ms"]).all() and np.isfinite(c["terms"]).all() and np.isfinite(c["mse"]).all() for c in table())


def test_ms_ssim_per_image_against_float64():
    """gate 1: |device - float64| <= 4 x max over the table of |host fp32 - float64|, and <= 1e-4 relative"""
    bound = 4 * max(c["host_err"] for c in table())
    worst = 0.0
    for c in table():
        err = float(np.abs(c["ms"] - c["exact"]).max())
        worst = max(worst, err)
        print(f"[ms-ssim] {c['what']:44s} float64 {c['exact'].mean():.9f}  |device - f64| {err:.2e}  |host fp32 - f64| {c['host_err']:.2e}")
        f64_gate(c["ms"], c["exact"], c["host_err"], f"ms_ssim {c['what']}", floor=0.0)
    print(f"[ms-ssim] table: device worst {worst:.2e}, bound 4 x host fp32 maximum = {bound:.2e}")
    for c in table():
        assert np.abs(c["ms"] - c["exact"]).max() <= bound, (c["what"], c["ms"], c["exact"], bound)


def test_terms_against_float64():
    """gate 2: every clamped per-scale mean, same rule (a pooling or halo mistake on scale 4 shows here, not in the product)"""
    bound = 4 * max(c["host_terms_err"] for c in table())
    for c in table():
        err = np.abs(c["terms"] - c["exact_terms"])
        print(f"[terms] {c['what']:44s} |device - f64| per scale {err.max(axis=(0, 1))}  |host fp32 - f64| {c['host_terms_err']:.2e}")
        f64_gate(c["terms"], c["exact_terms"], c["host_terms_err"], f"terms {c['what']}")
    print(f"[terms] bound 4 x host fp32 maximum = {bound:.2e}")
    for c in table():
        assert np.abs(c["terms"] - c["exact_terms"]).max() <= bound, (c["what"], np.abs(c["terms"] - c["exact_terms"]).max(axis=(0, 1)), bound)


def test_mse_against_float64():
    """gate 3: an fp64 sum of exact squares, rounded to fp32 once"""
    for c in table():
        print(f"[mse] {c['what']:44s} float64 {c['exact_mse']}  device {c['mse']}")
        assert np.all(np.abs(c["mse"] - c["exact_mse"]) <= 1e-6 * np.abs(c["exact_mse"])), (c["what"], c["mse"], c["exact_mse"])


def test_identical_inputs_give_one():
    """gate 4"""
    hit = [c for c in table() if " identical " in c["what"]]
    assert len(hit) == len(SIZES)
    for c in hit:
        assert np.abs(c["ms"] - 1.0).max() <= 1e-6, (c["what"], c["ms"])
        assert np.all(c["mse"] == 0.0)


def test_symmetric_bit_for_bit():
    """gate 5: ms_ssim(x, y) == ms_ssim(y, x); the kernel evaluates every expression that mixes x and y without fused contraction"""
    for c in table():
        a, b = device_run(c["x"], c["y"], c["data_range"]), device_run(c["y"], c["x"], c["data_range"])
        for u, v, name in zip(a, b, ("ms_ssim", "mse", "terms")):
            assert torch.equal(u, v), (c["what"], name)


@pytest.mark.parametrize("batch", [1, 8])
def test_two_calls_are_bit_identical_at_1080p(batch):
    """gate 6"""
    base = natural(1, 3, 1080, 1920, seed=3)
    x = torch.cat([torch.roll(base, (17 * k, 37 * k), dims=(2, 3)) for k in range(batch)])
    y = (x + 0.02 * torch.randn(x.shape, generator=torch.Generator().manual_seed(11))).clamp(0, 1)
    dev = torch.device("cuda:0")
    x, y = x.to(dev), y.to(dev)
    from spatiotemporalentropymodel_amd import functional as F
    first = [t.clone() for t in F.ms_ssim(x, y, return_terms=True)]
    second = F.ms_ssim(x, y, return_terms=True)
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    assert first[0].shape == (batch,) and first[1].shape == (batch,) and first[2].shape == (batch, 3, 5)
    assert bool(((first[0] > 0) & (first[0] < 1)).all())


def test_an_image_of_a_batch_equals_that_image_alone():
    """gate 7"""
    for c in table():
        if c["x"].shape[0] == 1:
            continue
        ms, mse, terms = device_run(c["x"], c["y"], c["data_range"])
        for b in range(c["x"].shape[0]):
            ms1, mse1, terms1 = device_run(c["x"][b:b + 1], c["y"][b:b + 1], c["data_range"])
            assert torch.equal(ms[b:b + 1], ms1) and torch.equal(mse[b:b + 1], mse1) and torch.equal(terms[b:b + 1], terms1), (c["what"], b)


def test_no_fifth_scale():
    """gate 8"""
    from spatiotemporalentropymodel_amd import evaluation, functional as F
    x = torch.rand(1, 3, 160, 160, device="cuda:0")
    with pytest.raises(ValueError):
        F.ms_ssim(x, x)
    with pytest.raises(ValueError):
        F.ms_ssim(torch.rand(1, 3, 300, 160, device="cuda:0"), torch.rand(1, 3, 300, 160, device="cuda:0"))
    assert evaluation.ms_ssim_device(x, x) is None
    big = torch.rand(2, 3, 161, 200, device="cuda:0")
    assert abs(evaluation.ms_ssim_device(big, big) - 1.0) <= 1e-6


def test_ms_ssim_device_averages_batch_and_channels():
    from spatiotemporalentropymodel_amd import evaluation
    c = next(c for c in table() if c["x"].shape[0] == 2 and "noise .05" in c["what"])
    got = evaluation.ms_ssim_device(c["x"].to("cuda:0"), c["y"].to("cuda:0"))
    assert isinstance(got, float) and abs(got - float(c["exact"].mean())) <= 4 * max(k["host_err"] for k in table())


def test_eval_gop_with_device_metrics(golden, monkeypatch):
    """gate 9: I + 2 P of seeded 176 x 208 frames, closed-form weights.  with_msssim="device" codes exactly what with_msssim=False
    codes, reports the kernel's MS-SSIM and PSNR, and does so with evaluation.ms_ssim / evaluation.psnr patched to raise: the host
    route provably does not run."""
    from spatiotemporalentropymodel_amd import evaluation
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    from test_hip_codec import _eval_gop_models
    dev = torch.device("cuda:0")
    imodel, stem = _eval_gop_models(golden("eval_gop.npz"), dev)
    frames = [f[0, :, 40:40 + 176, 24:24 + 208].contiguous().to(dev) for f in smooth_frames("msssim-gop", 1, 3, 256)]
    plain = evaluation.eval_gop(imodel, stem, frames, gop=12, with_msssim=False)
    host_run = evaluation.eval_gop(imodel, stem, frames, gop=12, with_msssim=True)
    host_psnr = [evaluation.psnr(x.unsqueeze(0), f["x_hat"]) for x, f in zip(frames, host_run["frames"])]

    def refuse(*a, **k):
        raise AssertionError("the host metric ran in a with_msssim='device' evaluation")
    monkeypatch.setattr(evaluation, "ms_ssim", refuse)
    monkeypatch.setattr(evaluation, "psnr", refuse)
    got = evaluation.eval_gop(imodel, stem, frames, gop=12, with_msssim="device")
    monkeypatch.undo()

    assert [f["type"] for f in got["frames"]] == ["I", "P", "P"]
    assert got["msssim_ave"] is not None and plain["msssim_ave"] is None
    bound = 4 * max(c["host_err"] for c in table())
    for t, (f, p, h, x) in enumerate(zip(got["frames"], plain["frames"], host_run["frames"], frames)):
        assert set(f) == set(p)
        assert f["strings"] == p["strings"] and f["bpp"] == p["bpp"] and tuple(f["shape"]) == tuple(p["shape"])
        assert torch.equal(f["y_conditioned"], p["y_conditioned"]) and torch.equal(f["x_hat"], h["x_hat"])
        exact, _ = ms_ssim_terms(x.unsqueeze(0).cpu(), f["x_hat"].cpu(), 1.0, torch.float64)
        exact_psnr = -10 * math.log10(float(((x.unsqueeze(0).double() - f["x_hat"].double()) ** 2).mean()))
        print(f"[eval_gop] frame {t}: ms-ssim device {f['ms-ssim']:.9f} host {h['ms-ssim']:.9f} float64 {float(exact[0]):.9f}   "
              f"psnr device {f['psnr']:.6f} host {host_psnr[t]:.6f} float64 {exact_psnr:.6f}")
        assert abs(f["ms-ssim"] - float(exact[0])) <= bound and abs(f["ms-ssim"] - float(exact[0])) <= 1e-4 * float(exact[0])
        assert abs(f["ms-ssim"] - h["ms-ssim"]) <= bound + abs(h["ms-ssim"] - float(exact[0]))
        assert abs(f["psnr"] - host_psnr[t]) <= 1e-4
        assert abs(f["psnr"] - exact_psnr) <= 1e-4
    assert abs(got["msssim_ave"] - sum(f["ms-ssim"] for f in got["frames"]) / 3) < 1e-12
    assert got["bpp_ave"] == plain["bpp_ave"]
