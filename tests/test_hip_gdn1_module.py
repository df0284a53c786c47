"""GPU, module and model level: layers.GDN1, FusedSequential around it, a FactorizedPrior whose GDNs are GDN1s, and ops.ste_round,
against the reference's own runs (tests/golden/gdn1.npz, make_golden_gdn1.py).

Float64 gates are conftest.f64_gate: 1e-4 of the exact value (floor 0.1), the reference's own fp32 distance printed next to ours.
Gradients of the model are megabytes: the fixture holds, per tensor, (sum, sum |.|) and a strided slice of 64 elements (the rule of
tests/test_hip_bmshj_models.py); the slice goes through f64_gate, the sums are held to 1e-4 x sum |.|."""
import numpy as np
import pytest
import torch

from conftest import f64_gate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.detach().cpu().contiguous().numpy()


@pytest.mark.parametrize("name", ["c32", "c36i"])
def test_module_matches_the_reference_module(golden, name):
    from spatiotemporalentropymodel_amd.layers import GDN1
    g = golden("gdn1.npz")
    pre = f"case:{name}:"
    C, inverse, _, _ = (int(v) for v in g[pre + "cfg"])
    m = GDN1(C, inverse=bool(inverse)).to(DEV)
    sd = m.state_dict()
    sd["beta"], sd["gamma"] = torch.from_numpy(g[pre + "beta"]), torch.from_numpy(g[pre + "gamma"])
    m.load_state_dict(sd)
    x = torch.from_numpy(g[pre + "x"]).to(DEV).requires_grad_(True)
    y = m(x)
    y.backward(torch.from_numpy(g[pre + "dy"]).to(DEV))
    for k, ours in (("y", y), ("dx", x.grad), ("dbeta", m.beta.grad), ("dgamma", m.gamma.grad)):
        assert tuple(ours.shape) == g[pre + k].shape
        f64_gate(host(ours), g[pre + k], g[pre + "ref32:" + k], f"GDN1 {name}: {k}")
    # only what is asked for is computed: a frozen module still hands dx on, a constant input still trains the module
    for p in m.parameters():
        p.requires_grad_(False)
    x2 = x.detach().clone().requires_grad_(True)
    m(x2).backward(torch.from_numpy(g[pre + "dy"]).to(DEV))
    assert torch.equal(x2.grad, x.grad)
    for p in m.parameters():
        p.requires_grad_(True)
        p.grad = None
    m(x.detach()).backward(torch.from_numpy(g[pre + "dy"]).to(DEV))
    f64_gate(host(m.gamma.grad), g[pre + "dgamma"], g[pre + "ref32:dgamma"], f"GDN1 {name}: dgamma without dx")


@pytest.mark.parametrize("grad", [False, True])
def test_fused_sequential_runs_a_gdn1_as_its_children_one_by_one(grad):
    from spatiotemporalentropymodel_amd import layers as L
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_, smooth_frames
    seq = closed_form_fill_(L.FusedSequential(L.conv(3, 32), L.GDN1(32), L.conv(32, 32), L.GDN1(32, inverse=True))).to(DEV)
    x = smooth_frames("gdn1:sequential", 1, 1, 64)[0].to(DEV)
    with torch.set_grad_enabled(grad):
        fused = seq(x)
        one = x
        for child in seq:
            one = child(one)
    assert fused.requires_grad == grad
    assert torch.equal(fused, one) and bool(torch.isfinite(fused).all()) and float(fused.detach().abs().max()) > 0


def _swap_gdn1(m):
    from spatiotemporalentropymodel_amd.layers import GDN, GDN1
    for seq in (m.g_a, m.g_s):
        for i, child in enumerate(seq):
            if isinstance(child, GDN):
                new = GDN1(child.beta.numel(), inverse=child.inverse)
                new.load_state_dict(child.state_dict())
                seq[i] = new
    return m


def _built(g):
    """make_golden_gdn1.build_gdn1 on this package's classes, the reference's tables loaded as a checkpoint brings them"""
    from spatiotemporalentropymodel_amd import models
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    gain, g_s_scale = float(g["model:gain"][0]), float(g["model:g_s_scale"][0])
    m = closed_form_fill_(models.FactorizedPrior(*(int(v) for v in g["model:NM"])))
    with torch.no_grad():
        m.g_a[6].weight.mul_(gain)
        m.g_a[6].bias.mul_(gain)
        m.g_s[0].weight.mul_(g_s_scale)
    m = _swap_gdn1(m).to(DEV).eval()
    assert m.update(force=True) is True
    sd = m.state_dict()
    assert [f"{k}|{','.join(map(str, v.shape))}" for k, v in sd.items()] == list(map(str, g["model:names"]))
    for k in ("entropy_bottleneck._quantized_cdf", "entropy_bottleneck._offset", "entropy_bottleneck._cdf_length"):
        ref = g["model:" + k]
        if k.endswith("_quantized_cdf"):
            diff = np.abs(host(sd[k]).astype(np.int64) - ref)
            assert diff.max() <= 1 and (diff != 0).mean() < 5e-3, k
        else:
            assert np.array_equal(host(sd[k]), ref), k
        sd[k] = torch.from_numpy(ref).to(DEV)
    m.load_state_dict(sd)
    return m


def _image(g):
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    h, w = (int(v) for v in g["model:size"])
    return smooth_frames(str(g["model:seed"][0]), 1, 1, max(h, w))[0][:, :, :h, :w].contiguous().to(DEV)


_MODEL = {}


def _model(golden):
    if not _MODEL:
        g = golden("gdn1.npz")
        _MODEL["m"] = (_built(g), g)
    return _MODEL["m"]


def test_swapped_model_eval_forward_matches_float64(golden):
    from spatiotemporalentropymodel_amd.layers import GDN1
    m, g = _model(golden)
    assert sum(isinstance(c, GDN1) for c in list(m.g_a) + list(m.g_s)) == 6
    with torch.no_grad():
        fwd = m(_image(g))
    for k, ours in (("y_hat", fwd["y_hat"]), ("lik_y", fwd["likelihoods"]["y"]), ("x_hat", fwd["x_hat"]), ("y", fwd["y"])):
        f64_gate(host(ours), g["model:fwd:" + k], g["model:ref32:" + k], f"FactorizedPrior on GDN1: forward {k}", atol=1e-9 if k == "lik_y" else 0.0)


def test_swapped_model_codes_the_reference_bytes(golden):
    m, g = _model(golden)
    x = _image(g)
    print(f"[margin] y - median from a half-integer: {float(g['model:margin'][0]):.2e} = "
          f"{float(g['model:margin'][0]) / float(g['model:margin_ref32'][0]):.0f} x the reference's fp32 distance")
    assert float(g["model:margin"][0]) >= float(g["model:margin_factor"][0]) * float(g["model:margin_ref32"][0])
    want = g["model:y_string"].tobytes()
    enc = m.compress(x)
    assert tuple(enc["shape"]) == tuple(g["model:shape"]) and len(enc["strings"]) == 1 and len(enc["strings"][0]) == 1
    ours = enc["strings"][0][0]
    n = min(len(ours), len(want))
    assert ours == want, f"lengths {len(ours)} / {len(want)}, first differing byte {next((j for j in range(n) if ours[j] != want[j]), n)}"
    dec = m.decompress(enc["strings"], enc["shape"])
    with torch.no_grad():
        fwd = m(x)
    assert torch.equal(dec["y_hat"], fwd["y_hat"])
    # the encoder-side reconstruction: g_s of the symbols the encoder coded, clamped as decompress clamps
    assert torch.equal(dec["x_hat"], fwd["x_hat"].clamp(0, 1))
    pre = max(float(np.abs(g["model:fwd:x_hat"]).max()), 1.0)       # a pixel next to a clamp edge carries the unclamped tensor's error
    f64_gate(host(dec["x_hat"]), g["model:x_hat"], g["model:ref32:x_hat"], "FactorizedPrior on GDN1: decoded image", atol=1e-4 * pre)


def test_swapped_model_training_gradients_match_float64(golden):
    from spatiotemporalentropymodel_amd.losses import RateDistortionLoss
    from spatiotemporalentropymodel_amd.selfcheck import NoiseFeed
    m, g = _model(golden)
    x = _image(g)
    m.train()
    try:
        m.entropy_bottleneck.noise_source = NoiseFeed("gdn1:factorized:grad_eb")
        for p in m.parameters():
            p.grad = None
        oc = RateDistortionLoss(lmbda=float(g["model:hyper"][0]))(m(x), x)
        oc["loss"].backward()
        torch.cuda.synchronize()
    finally:
        m.entropy_bottleneck.noise_source = None
        m.eval()
    want = dict(zip(map(str, g["model:scalar_names"]), zip(g["model:scalars"], g["model:scalars_ref32"])))
    for k in ("loss", "mse_loss", "bpp_loss"):
        ref, r32 = want[k]
        print(f"[gdn1 model] {k}: {float(oc[k]):.8g} (float64 {ref:.8g}; reference fp32 {r32:.1e})")
        assert abs(float(oc[k]) - ref) <= 1e-4 * abs(ref), (k, float(oc[k]), ref)
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    keys = list(map(str, g["model:grad_keys"]))
    assert sorted(grads) == sorted(keys)
    n = int(g["model:slice"][0])
    for k in keys:
        flat = grads[k].detach().double().reshape(-1)
        sums, sl, r32 = g[f"model:sum:{k}"], g[f"model:slice:{k}"], g[f"model:ref32:d:{k}"]
        assert flat.numel() == int(sums[3]), k
        assert abs(float(flat.sum()) - sums[0]) <= 1e-4 * sums[1] + 1e-300, (k, float(flat.sum()), sums[0], sums[1], float(r32[1]))
        assert abs(float(flat.abs().sum()) - sums[1]) <= 1e-4 * sums[1] + 1e-300, (k, float(flat.abs().sum()), sums[1], float(r32[1]))
        f64_gate(host(flat[:: max(1, flat.numel() // n)][:n]), sl, r32[:1], f"FactorizedPrior on GDN1: gradient of {k}")


def test_ste_round_rounds_half_to_even_and_passes_the_gradient():
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd.ops import ste_round
    rng = np.random.default_rng(5)
    v = rng.uniform(-40, 40, (2, 7, 5, 6)).astype(np.float32)
    f = v.reshape(-1)
    f[0::7] = np.arange(f[0::7].size, dtype=np.float32) - 30.5          # exact half-integer ties on both sides of zero
    f[1::7] = np.float32(-0.0)
    f[2::7] = rng.uniform(-0.49, 0.49, f[2::7].size).astype(np.float32)   # round to +0.0 and to -0.0
    for name, x in (("NCHW", torch.from_numpy(v).to(DEV)), ("NHWC", torch.from_numpy(v).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)),
                    ("flat", torch.from_numpy(f.copy()).to(DEV))):
        x = x.requires_grad_(True)
        y = ste_round(x)
        assert y.stride() == x.stride() and y.shape == x.shape, name
        assert np.array_equal(host(y).view(np.int32), np.rint(host(x)).view(np.int32)), f"{name}: not numpy.rint bit for bit"
        gy = torch.from_numpy(rng.normal(0, 1, tuple(x.shape)).astype(np.float32)).to(DEV)
        y.backward(gy)
        assert np.array_equal(host(x.grad).view(np.int32), host(gy).view(np.int32)), f"{name}: the gradient was changed"
    # a channel-slice view (gaps in memory) is rounded too
    buf = F.empty_nhwc(1, 12, 4, 4, DEV)
    buf.copy_(torch.from_numpy(rng.uniform(-9, 9, (1, 12, 4, 4)).astype(np.float32)))
    assert np.array_equal(host(ste_round(buf[:, 2:7])), np.rint(host(buf[:, 2:7])))
