#!/usr/bin/env python3
"""Generate tests/golden/gdn1.npz from the REFERENCE itself (compressai/layers/gdn.py:70-96: GDN1; compressai/models/priors.py:109-170:
FactorizedPrior), run as it is on the CPU.  See make_golden.py for the import recipe, make_golden_bmshj.py for the model recipe
(`build`) and the margin rule this follows.

    python tests/golden/make_golden_gdn1.py

  layers_all, ops_all       compressai.layers.__all__ and compressai.ops.__all__, as data
  case:<name>:*             the reference's GDN1 module per CASES entry: a fresh module's state dict (init:<key>), then stored parameters
                            on both sides of their bounds, an input with both signed zeros and an incoming gradient: x, dy, beta, gamma
                            (float32, what the float64 run was fed) and y, dx, dbeta, dgamma of the float64 run rounded to float32,
                            with the fp32 run's distance ref32:<tensor> (conftest.close_ratio, floor 0.1)
  model:*                   FactorizedPrior(64, 96) built as make_golden_bmshj.build builds it, every GDN of g_a / g_s replaced by a GDN1
                            carrying the same parameters, on one 128 x 128 image: the ordered state-dict names with shapes, the CDF
                            tables, the eval forward in float64 (y_hat, lik_y, x_hat) with the fp32 distance, the compress string,
                            decompress's x_hat, the margin; and in training mode, noise fed by name (make_golden.NoiseFeed), the terms of
                            RateDistortionLoss(lmbda=1e-2) and a digest of the gradient of every parameter -- (sum, sum |.|, sum of
                            squares, count) and a strided slice, as bmshj_train.npz holds them -- float64 with the fp32 distance

Margin.  The only threshold of the factorized model is the bottleneck's rounding: candidates (gain, image seed) are tried in a fixed
order and the first is kept whose distance of y - median from a half-integer is at least MARGIN_FACTOR x the reference's own
fp32-vs-float64 distance on that tensor (asserted).  The image is regenerated from its seed name, not stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import NoiseFeed, import_reference, save, t2n  # noqa: E402
from make_golden_bmshj import GAINS, G_S_SCALE, NM, NSEEDS, SLICE, LMBDA, build, digest, rd_loss  # noqa: E402
from make_golden_cheng import MARGIN_FACTOR, close_ratio, half_integer_margin, image  # noqa: E402

#: name, channels, inverse, (H, W)
CASES = (("c5", 5, False, (3, 7)), ("c32", 32, False, (9, 8)), ("c36i", 36, True, (10, 13)))
SIZE = (128, 128)
TABLES = ("entropy_bottleneck._quantized_cdf", "entropy_bottleneck._offset", "entropy_bottleneck._cdf_length")
FWD = ("y", "y_hat", "x_hat", "lik_y")


def case_inputs(name, C, hw):
    rng = np.random.default_rng(sum(map(ord, name)))
    n = hw[0] * hw[1]
    x = (np.logspace(-2, 1, C)[None, :] * rng.uniform(0.5, 1.0, (n, C)) * rng.choice([-1.0, 1.0], (n, C))).astype(np.float32)
    x.reshape(-1)[4::11] = 0.0
    x.reshape(-1)[9::13] = -0.0
    dy = rng.normal(0, 1, (n, C)).astype(np.float32)
    gamma = np.sqrt(rng.uniform(0.5, 1.5, (C, C)) / C).astype(np.float32)
    gamma.reshape(-1)[3::14] = 1e-6
    gamma.reshape(-1)[10::14] = -0.3
    beta = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta[2::10] = 1e-4
    beta[7::10] = 0.0
    to_nchw = lambda a: np.ascontiguousarray(a.reshape(1, hw[0], hw[1], C).transpose(0, 3, 1, 2))      # noqa: E731
    return to_nchw(x), to_nchw(dy), beta, gamma


def run_case(C, inverse, x, dy, beta, gamma, dtype):
    from compressai.layers import GDN1
    m = GDN1(C, inverse=inverse).to(dtype)
    with torch.no_grad():
        m.beta.copy_(torch.from_numpy(beta))
        m.gamma.copy_(torch.from_numpy(gamma))
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = m(xt)
    y.backward(torch.from_numpy(dy).to(dtype))
    return {"y": t2n(y), "dx": t2n(xt.grad), "dbeta": t2n(m.beta.grad), "dgamma": t2n(m.gamma.grad)}


def gen_cases(d):
    from compressai.layers import GDN1
    for name, C, inverse, hw in CASES:
        x, dy, beta, gamma = case_inputs(name, C, hw)
        pre = f"case:{name}:"
        d[pre + "cfg"] = np.array([C, int(inverse), hw[0], hw[1]])
        sd = GDN1(C, inverse=inverse).state_dict()
        d[pre + "init_keys"] = np.array(list(sd))
        for k, v in sd.items():
            d[pre + "init:" + k] = t2n(v)
        d.update({pre + "x": x, pre + "dy": dy, pre + "beta": beta, pre + "gamma": gamma})
        r64, r32 = run_case(C, inverse, x, dy, beta, gamma, torch.float64), run_case(C, inverse, x, dy, beta, gamma, torch.float32)
        for k in r64:
            d[pre + k] = r64[k].astype(np.float32)
            d[pre + "ref32:" + k] = np.array([close_ratio(r32[k], r64[k])])
        print(f"case {name}: reference fp32 vs float64 " + ", ".join(f"{k} {float(d[pre + 'ref32:' + k][0]):.1e}" for k in r64))


def swap_gdn1(m):
    """every GDN of g_a / g_s -> a GDN1 carrying the same parameters"""
    from compressai.layers import GDN, GDN1
    for seq in (m.g_a, m.g_s):
        for i, child in enumerate(seq):
            if isinstance(child, GDN):
                new = GDN1(child.beta.numel(), inverse=child.inverse).to(child.beta.dtype)
                new.load_state_dict(child.state_dict())
                seq[i] = new
    return m


def build_gdn1(gain, dtype=torch.float32):
    from compressai.models.priors import FactorizedPrior
    m = swap_gdn1(build(FactorizedPrior, gain)).to(dtype).eval()
    m.update(force=True)
    return m


def eval_forward(m, x):
    with torch.no_grad():
        out = m(x)
        y = m.g_a(x)
        med = m.entropy_bottleneck._get_medians().detach().reshape(1, -1, 1, 1)
        return {"y": t2n(y), "y_hat": t2n(m.entropy_bottleneck(y)[0]), "x_hat": t2n(out["x_hat"]), "lik_y": t2n(out["likelihoods"]["y"]),
                "y_centered": t2n(y - med)}


def choose():
    for gain in GAINS:
        m32, m64 = build_gdn1(gain), build_gdn1(gain, torch.float64)
        for s in range(NSEEDS):
            seed = f"gdn1:factorized:{SIZE[0]}x{SIZE[1]}:{s}"
            x = image(seed, SIZE)
            f32, f64 = eval_forward(m32, x), eval_forward(m64, x.double())
            margin, dist = half_integer_margin(f64["y_centered"]), float(np.abs(f32["y_centered"] - f64["y_centered"]).max())
            if margin >= MARGIN_FACTOR * dist:
                return gain, seed, m32, f32, f64, margin, dist
        print(f"  gain {gain}: no seed clears {MARGIN_FACTOR:.0f} x")
    raise AssertionError("no candidate clears the margin factor: change GAINS or the seeds, not a gate")


def train_run(gain, seed, dtype):
    m = build_gdn1(gain, dtype).train()
    m.entropy_bottleneck._get_noise_cached = NoiseFeed("gdn1:factorized:grad_eb", [])
    x = image(seed, SIZE).to(dtype)
    oc = rd_loss(m(x), x)
    oc["loss"].backward()
    return {k: float(v.detach()) for k, v in oc.items()}, {n: digest(p.grad) for n, p in m.named_parameters() if p.grad is not None}


def gen_model(d):
    gain, seed, m, f32, f64, margin, dist = choose()
    x = image(seed, SIZE)
    with torch.no_grad():
        enc = m.compress(x)
        dec = m.decompress(enc["strings"], enc["shape"])
    sd = m.state_dict()
    d.update({"model:gain": np.array([gain]), "model:g_s_scale": np.array([G_S_SCALE / gain]), "model:NM": np.array(NM), "model:seed": np.array([seed]),
              "model:size": np.array(SIZE), "model:margin_factor": np.array([MARGIN_FACTOR]), "model:margin": np.array([margin]),
              "model:margin_ref32": np.array([dist]), "model:names": np.array([f"{k}|{','.join(map(str, v.shape))}" for k, v in sd.items()]),
              "model:y_string": np.frombuffer(enc["strings"][0][0], dtype=np.uint8), "model:shape": np.array(enc["shape"]),
              "model:x_hat": t2n(dec["x_hat"])})
    for k in TABLES:
        d["model:" + k] = t2n(sd[k]).astype(np.int32)
    for k in FWD:
        d["model:fwd:" + k] = f64[k].astype(np.float32)
        d["model:ref32:" + k] = np.array([close_ratio(f32[k], f64[k])])
    print(f"model: gain {gain}, {seed}: string {len(enc['strings'][0][0])} B, y_hat non-zero {float((f64['y_hat'] != 0).mean()):.2f}, |y| max "
          f"{np.abs(f64['y']).max():.2f}, margin {margin:.3e} = {margin / max(dist, 1e-300):.0f} x the fp32 distance {dist:.3e}")
    print("    reference fp32 vs float64: " + ", ".join(f"{k} {float(d['model:ref32:' + k][0]):.1e}" for k in FWD))
    s64, r64 = train_run(gain, seed, torch.float64)
    s32, r32 = train_run(gain, seed, torch.float32)
    d["model:hyper"], d["model:slice"] = np.array([LMBDA]), np.array([SLICE])
    d["model:scalar_names"] = np.array(list(s64))
    d["model:scalars"] = np.array([s64[k] for k in s64])
    d["model:scalars_ref32"] = np.array([abs(s32[k] - s64[k]) / max(abs(s64[k]), 1e-300) for k in s64])
    d["model:grad_keys"] = np.array(list(r64))
    worst = 0.0
    for k, (sums, sl) in r64.items():
        d[f"model:sum:{k}"], d[f"model:slice:{k}"] = sums, sl
        d[f"model:ref32:d:{k}"] = np.array([close_ratio(r32[k][1], sl) if np.abs(sl).max() > 0 else 0.0,
                                            float(np.abs(r32[k][0][:2] - sums[:2]).max() / max(sums[1], 1e-300))])
        worst = max(worst, float(d[f"model:ref32:d:{k}"][0]))
    print("train: " + ", ".join(f"{k} {v:.6g}" for k, v in s64.items()) + f"; {len(r64)} gradient digests, reference fp32 vs float64 at most {worst:.1e}")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    import_reference()
    import compressai.layers
    import compressai.ops
    d = {"layers_all": np.array(list(compressai.layers.__all__)), "ops_all": np.array(list(compressai.ops.__all__))}
    gen_cases(d)
    gen_model(d)
    save("gdn1.npz", d)
