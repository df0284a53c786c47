"""GPU: stem_ms_ssim_bwd (csrc/msssim.hip) through functional.ms_ssim_backward, losses.ms_ssim and
RateDistortionLoss(metric="ms-ssim").

Yardstick: float64 torch-CPU autograd through the algorithm evaluation.ms_ssim defines (its body with the same fp32-rounded window;
`ms_ssim_terms`, `natural` and `distorted` are tests/test_hip_msssim.py's helpers, the first one returning tensors here so that
autograd can run through it).  The upstream gradient is linspace(0.5, 1.5, B): not uniform, so a per-image scaling mistake shows.
The fp32 autograd run of the same body is the scale of the bound: per image, max|dx_device - dx_f64| must be within 1e-4 of that
image's max|dx_f64| (the project's tolerance) and no worse than the LARGEST fp32-reference error of this run's table.  On the CPU
the table gave: smallest term 0.55 .. 0.97 (no clamp active), max|grad| per image 2.4e-5 .. 6e-4 (9.5e-8 at data_range 255), fp32
reference error relative to the image's max|grad| 9e-6 .. 8.9e-5.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SHAPES = [(1, 3, 161, 161), (2, 3, 177, 211), (3, 1, 192, 320)]
DISTORTIONS = ["noise .01", "noise .05", "blur", "quant 5 bit"]
CASES = [(shape, name, 1.0) for shape in SHAPES for name in DISTORTIONS] + [((1, 3, 256, 256), "noise .01", 255.0)]
RTOL = 1e-4


def _filter(x, k):
    C = x.shape[1]
    x = torch.nn.functional.conv2d(x, k.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return torch.nn.functional.conv2d(x, k.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)


def ms_ssim_terms(x, y, data_range, dtype):
    """the body of evaluation.ms_ssim in `dtype`, window rounded to fp32 first -> (per image [B], clamped per-scale means [B,C,5]),
    both tensors of `dtype` with the graph attached"""
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
    return torch.prod(t ** w, dim=0).mean(1), t.permute(1, 2, 0)


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
    assert name == "quant 5 bit"
    return x, torch.round(x * 31) / 31


def upstream(B):
    return torch.linspace(0.5, 1.5, B)


def host_grad(x, y, data_range, dtype, grad_ms):
    """autograd through the body in `dtype` -> (dx as float64 numpy, the smallest clamped term)"""
    xr = x.detach().to(dtype).clone().requires_grad_(True)            # a copy: the images are shared among the cases
    ms, terms = ms_ssim_terms(xr, y, data_range, dtype)
    ms.backward(grad_ms.to(dtype))
    return xr.grad.double().numpy(), float(terms.detach().min())


def device_grad(x, y, grad_ms, data_range=1.0):
    from spatiotemporalentropymodel_amd import functional as F
    dev = torch.device("cuda:0")
    return F.ms_ssim_backward(x.to(dev), y.to(dev), grad_ms.to(dev), data_range)


def per_image_max(a):
    return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


@functools.lru_cache(maxsize=None)
def table():
    """every case once: inputs, the float64 and the fp32 autograd gradients, the device gradient"""
    cases = []
    for shape, name, data_range in CASES:
        base = natural(*shape, seed=1)
        x, y = distorted(base, name, torch.Generator().manual_seed(7))
        x, y = (x * data_range).contiguous(), (y * data_range).contiguous()
        g = upstream(shape[0])
        exact, smallest = host_grad(x, y, data_range, torch.float64, g)
        host32, _ = host_grad(x, y, data_range, torch.float32, g)
        dx = device_grad(x, y, g, data_range)
        scale = per_image_max(exact)
        cases.append({"what": f"{'x'.join(map(str, shape))} {name} range {data_range:g}", "shape": shape, "name": name, "x": x, "y": y, "g": g,
                      "data_range": data_range, "exact": exact, "scale": scale, "smallest_term": smallest,
                      "host_err": per_image_max(host32 - exact) / scale, "dx": dx, "dev_err": per_image_max(dx.double().cpu().numpy() - exact) / scale})
    return cases


def test_every_case_is_in_the_table():
    assert len(table()) == len(SHAPES) * len(DISTORTIONS) + 1 == 13
    for c in table():
        assert c["smallest_term"] > 0.0, (c["what"], "a clamp is active: the float64 gradient is not the yardstick of this case")
        assert tuple(c["dx"].shape) == c["shape"] and c["dx"].dtype == torch.float32 and bool(torch.isfinite(c["dx"]).all())
        assert np.all(c["scale"] > 0)


def test_gradient_against_float64():
    """gate 1: per image, max|device - f64| <= 1e-4 max|f64|, and no worse than the largest fp32-reference error of the table"""
    host_worst = max(float(c["host_err"].max()) for c in table())
    for c in table():
        print(f"[ms-ssim grad] {c['what']:40s} max|grad| {c['scale'].max():.2e}  smallest term {c['smallest_term']:.3f}  "
              f"device {c['dev_err'].max():.2e}  fp32 reference {c['host_err'].max():.2e}  bound {RTOL:.0e}")
    print(f"[ms-ssim grad] table: device worst {max(float(c['dev_err'].max()) for c in table()):.2e}, fp32 reference worst {host_worst:.2e}")
    for c in table():
        assert np.all(c["dev_err"] <= RTOL), (c["what"], c["dev_err"])
        assert np.all(c["dev_err"] <= host_worst), (c["what"], c["dev_err"], host_worst)


def test_forward_is_untouched():
    """gate 2: losses.ms_ssim == functional.ms_ssim, bit for bit"""
    from spatiotemporalentropymodel_amd import functional as F, losses
    dev = torch.device("cuda:0")
    for c in table():
        x, y = c["x"].to(dev), c["y"].to(dev)
        want = F.ms_ssim(x, y, c["data_range"])[0]
        assert torch.equal(losses.ms_ssim(x, y, c["data_range"]), want), c["what"]
        assert torch.equal(losses.ms_ssim(x.clone().requires_grad_(True), y, c["data_range"]).detach(), want), c["what"]


def test_identical_inputs():
    """gate 3: at x == y every |dx| <= 1e-4 of the "noise .01" gradient's maximum (the smallest image's) of the same shape; all finite"""
    for c in table():
        if c["name"] != "noise .01":
            continue
        dx = device_grad(c["x"], c["x"].clone(), c["g"], c["data_range"])
        bound = RTOL * float(c["scale"].min())
        print(f"[ms-ssim grad] identical {c['what']:40s} max|dx| {float(dx.abs().max()):.2e}  bound {bound:.2e}")
        assert bool(torch.isfinite(dx).all())
        assert float(dx.abs().max()) <= bound, (c["what"], float(dx.abs().max()), bound)


def test_clamped_channels_give_exact_zeros():
    """gate 4: y = 1 - x on the 161 x 161 image: negative structure on every scale, at least one clamped term per channel"""
    from spatiotemporalentropymodel_amd import functional as F
    dev = torch.device("cuda:0")
    x = natural(1, 3, 161, 161, seed=1)
    y = (1 - x).contiguous()
    _, terms = ms_ssim_terms(x, y, 1.0, torch.float64)
    assert bool((terms.amin(dim=2) <= 0).all()), terms
    ms, _, dterms = F.ms_ssim(x.to(dev), y.to(dev), return_terms=True)
    assert bool((dterms.amin(dim=2) == 0).all()) and float(ms) == 0.0
    dx = device_grad(x, y, torch.ones(1))
    assert not bool(torch.isnan(dx).any()) and bool((dx == 0).all())

    # mixed: channel 0 clamped, channel 1 a "noise .05" pair.  Float64 for channel 1: the body on that channel alone, halved (C = 2)
    x1, y1 = distorted(x[:, 1:2], "noise .05", torch.Generator().manual_seed(7))
    xm, ym = torch.cat([x[:, :1], x1], 1).contiguous(), torch.cat([y[:, :1], y1], 1).contiguous()
    _, tm = ms_ssim_terms(xm, ym, 1.0, torch.float64)
    assert float(tm[0, 0].min()) <= 0 < float(tm[0, 1].min())
    g = torch.full((1,), 1.25)
    exact, _ = host_grad(x1, y1, 1.0, torch.float64, 0.5 * g)
    host32, _ = host_grad(x1, y1, 1.0, torch.float32, 0.5 * g)
    dx = device_grad(xm, ym, g)
    assert bool(torch.isfinite(dx).all()) and bool((dx[:, 0] == 0).all())
    err = np.abs(dx[:, 1:2].double().cpu().numpy() - exact).max() / np.abs(exact).max()
    print(f"[ms-ssim grad] mixed clamp, channel 1: device {err:.2e}  fp32 reference {np.abs(host32 - exact).max() / np.abs(exact).max():.2e}  bound {RTOL:.0e}")
    assert err <= RTOL and err <= max(float(c["host_err"].max()) for c in table())


def test_deterministic_and_independent_of_the_batch():
    """gate 5"""
    from spatiotemporalentropymodel_amd import losses
    dev = torch.device("cuda:0")
    for c in table():
        again = device_grad(c["x"], c["y"], c["g"], c["data_range"])
        assert torch.equal(again, c["dx"]), c["what"]
        B = c["shape"][0]
        for b in range(B if B > 1 else 0):
            one = device_grad(c["x"][b:b + 1], c["y"][b:b + 1], c["g"][b:b + 1], c["data_range"])
            assert torch.equal(one, c["dx"][b:b + 1]), (c["what"], b)
        # d ms(y_as_x_hat, x_as_target) / d target: the kernel with its arguments swapped
        t = c["x"].to(dev).requires_grad_(True)
        losses.ms_ssim(c["y"].to(dev), t, c["data_range"]).backward(c["g"].to(dev))
        assert torch.equal(t.grad, c["dx"]), c["what"]


def test_both_arguments_in_one_backward():
    """x_hat and target both leaves: each gets the gradient the functional call gives for it"""
    from spatiotemporalentropymodel_amd import losses
    dev = torch.device("cuda:0")
    c = next(c for c in table() if c["shape"] == (2, 3, 177, 211) and c["name"] == "blur")
    a, b = c["x"].to(dev).requires_grad_(True), c["y"].to(dev).requires_grad_(True)
    losses.ms_ssim(a, b).backward(c["g"].to(dev))
    assert torch.equal(a.grad, c["dx"]) and torch.equal(b.grad, device_grad(c["y"], c["x"], c["g"]))
    exact_b, _ = host_grad(c["y"], c["x"], 1.0, torch.float64, c["g"])
    assert np.all(per_image_max(b.grad.double().cpu().numpy() - exact_b) <= RTOL * per_image_max(exact_b))


def test_criterion_and_autograd():
    """gate 6"""
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd.losses import RateDistortionLoss, _WeightedMSEFunction, log2_sum
    dev = torch.device("cuda:0")
    c = next(c for c in table() if c["shape"] == (2, 3, 177, 211) and c["name"] == "noise .05")
    B, _, H, W = c["shape"]
    target = c["x"].to(dev)
    lik0 = (torch.rand(B, 8, 12, 14, generator=torch.Generator().manual_seed(5)) * 0.9 + 0.05).to(dev)

    def run(criterion):
        x_hat, lik = c["y"].to(dev).requires_grad_(True), lik0.clone().requires_grad_(True)
        out = criterion({"x_hat": x_hat, "likelihoods": {"y": lik}}, target)
        out["loss"].backward()
        return out, x_hat.grad, lik.grad

    out, gx, gl = run(RateDistortionLoss(lmbda=0.7, metric="ms-ssim"))
    assert set(out) == {"bpp_loss", "ms_ssim_loss", "loss"}
    ms = F.ms_ssim(c["y"].to(dev), target)[0]
    assert abs(float(out["ms_ssim_loss"]) - (1.0 - float(ms.double().mean()))) <= 2.0 ** -23
    assert abs(float(out["loss"]) - (0.7 * float(out["ms_ssim_loss"]) + float(out["bpp_loss"]))) <= 1e-6 * abs(float(out["loss"]))
    assert torch.equal(gx, F.ms_ssim_backward(c["y"].to(dev), target, torch.full((B,), -0.7 / B, device=dev)))

    # The scalars of the squared-error criterion and of the rate come from kernels that add their workgroups' fp64 partial sums
    # in arrival order (stem_weighted_sqerr_sum, stem_log2_sum: at most 1024 partials of one sign), so two runs agree to
    # 1024 * 2^-53 = 1.2e-13 relative, not bit for bit: they are held to 1e-12.  The gradients do not depend on those sums (their
    # upstream factors are constants of the criterion) and are compared bit for bit.
    def same_sum(a, b):
        return abs(float(a) - float(b)) <= 1e-12 * abs(float(b))

    out_mse, gx_mse, gl_mse = run(RateDistortionLoss(lmbda=0.7, metric="mse"))
    assert torch.equal(gl, gl_mse) and same_sum(out["bpp_loss"], out_mse["bpp_loss"])
    out_def, gx_def, gl_def = run(RateDistortionLoss(lmbda=0.7))
    assert set(out_mse) == set(out_def) == {"bpp_loss", "mse_loss", "loss"}
    for k in out_def:
        assert out_mse[k].dtype == out_def[k].dtype and same_sum(out_mse[k], out_def[k]), k
    assert torch.equal(gx_mse, gx_def) and torch.equal(gl_mse, gl_def)
    # today's formula, written out
    x_hat, lik = c["y"].to(dev).requires_grad_(True), lik0.clone().requires_grad_(True)
    mse = _WeightedMSEFunction.apply(x_hat, target, torch.ones(B, 1, H, W, device=dev))
    loss = 0.7 * 255 ** 2 * mse + log2_sum(lik) / (-B * H * W)
    loss.backward()
    assert same_sum(loss, out_def["loss"]) and same_sum(mse, out_def["mse_loss"])
    assert torch.equal(x_hat.grad, gx_def) and torch.equal(lik.grad, gl_def)
    exact_mse = float(((c["y"].double() - c["x"].double()) ** 2).mean())
    assert abs(float(mse) - exact_mse) <= 1e-5 * exact_mse


def test_no_fifth_scale():
    from spatiotemporalentropymodel_amd import functional as F, losses
    dev = torch.device("cuda:0")
    for shape in ((1, 3, 160, 160), (1, 3, 300, 160)):
        x = torch.rand(*shape, device=dev)
        with pytest.raises(ValueError):
            losses.ms_ssim(x.clone().requires_grad_(True), x)
        with pytest.raises(ValueError):
            F.ms_ssim_backward(x, x, torch.ones(1, device=dev))
        with pytest.raises(ValueError):
            losses.RateDistortionLoss(metric="ms-ssim")({"x_hat": x, "likelihoods": {"y": torch.rand(1, 4, 8, 8, device=dev) * 0.9 + 0.05}}, x)


def test_training_pass_of_the_variable_rate_iframe_model():
    """gate 7: one training forward / backward of stem_roi_i (the model tests/test_hip_roi.py trains; autograd drives its backward)
    on one 192 x 192 frame, closed-form weights, with RateDistortionLoss(metric="ms-ssim") in place of the squared-error criterion"""
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd.losses import RateDistortionLoss
    from spatiotemporalentropymodel_amd.models import stem_roi_i
    from spatiotemporalentropymodel_amd.selfcheck import NoiseFeed
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_scaled_, closed_form_input, smooth_frames
    dev = torch.device("cuda:0")
    m = closed_form_fill_scaled_(stem_roi_i(), "roi_i", 0.7).to(dev).train()
    m.entropy_bottleneck.noise_source = NoiseFeed("roi_i_eb")
    m.gaussian_conditional.noise_source = NoiseFeed("roi_i_gc")
    frame = smooth_frames("msssim-train", 1, 1, 192)[0].to(dev)
    qmap = closed_form_input("msssim-train:q", (1, 1, 192, 192)).to(dev)
    out = m(frame, qmap)
    assert tuple(out["x_hat"].shape) == (1, 3, 192, 192)
    caught = []
    out["x_hat"].register_hook(lambda t: caught.append(t.detach().clone()))
    oc = RateDistortionLoss(lmbda=0.7, metric="ms-ssim")(out, frame)
    terms = F.ms_ssim(out["x_hat"], frame, return_terms=True)[2]
    print(f"[ms-ssim grad] stem_roi_i 192 x 192: ms_ssim_loss {float(oc['ms_ssim_loss']):.6f}  smallest term {float(terms.min()):.4f}")
    oc["loss"].backward()
    assert len(caught) == 1
    assert torch.equal(caught[0], F.ms_ssim_backward(out["x_hat"], frame, torch.full((1,), -0.7, device=dev)))
    seen = 0
    for n, p in m.named_parameters():
        if n.startswith("gs") and n.endswith("weight"):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
            seen += 1
    assert seen >= 4
