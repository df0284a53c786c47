#!/usr/bin/env python3
"""Generate the fixture of EntropyBottleneck(filters != (3, 3, 3, 3)) from the REFERENCE itself
(compressai/entropy_models/entropy_models.py:282-475, run as it is on the CPU).  See make_golden.py for the import recipe,
make_golden_bmshj.py for the margin rule and the build of the FactorizedPrior.

    python tests/golden/make_golden_eb_filters.py

  eb_filters.npz, per tuple <t> of TUPLES (keys "<t>:...", <t> = "f3-3-3", "fnone" for ()), EntropyBottleneck(5, filters=<t>):
      names                 ordered state-dict keys with shapes
      init:<param>          the parameters as constructed after torch.manual_seed(SEED)
      sd:<key>              the state dict after closed_form_fill_ (every parameter perturbed, non-zero medians) and update(force=True):
                            parameters, quantiles, target, _quantized_cdf, _offset, _cdf_length
      x, w                  the [2, 5, 9, 11] input and the weights of z_hat in the scalar that is differentiated
      train:z_hat | lik     training forward, noise fed by name (make_golden.NoiseFeed, role "ebf:<t>"), float64
      eval:z_hat | lik      eval forward, float64
      grad:<param> | x      d / d(.) of  coef * sum(log2 lik) + sum(w * z_hat)  (training forward), float64
      aux, aux:dq           loss() and its gradient with respect to quantiles, float64
      ref32:<any of these>  the float32 run's distance (conftest.close_ratio, floor 0.1) from the float64 one
      string:<b>, dec       compress strings of x and decompress's output
      margin                (z - median from a half-integer, the reference's fp32-vs-float64 distance on z - median, candidate index)
  and, keys "fp:...", one FactorizedPrior(64, 96) whose entropy_bottleneck is EntropyBottleneck(96, filters=(3, 3, 3)), built and scaled
  as make_golden_bmshj.build does it, on one 128 x 128 image: the bottleneck's state dict, the eval forward in float64 (y_hat, lik_y,
  x_hat) with the fp32 run's distance, the string, decompress's x_hat, and the margin.

Byte identity is demanded under make_golden_bmshj.py's margin rule: candidates (input seeds; for the model (gain, image seed)) are
tried in a fixed order and the first is kept whose z - median stays at least MARGIN_FACTOR x the reference's own fp32-vs-float64
distance from a half-integer.  That one exists is asserted here.  Float64 tensors are stored rounded to float32.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import NoiseFeed, closed_form_fill_, closed_form_input, import_reference, save, t2n  # noqa: E402
from make_golden_bmshj import G_S_SCALE, GAINS, NM  # noqa: E402
from make_golden_cheng import MARGIN_FACTOR, close_ratio, half_integer_margin, image  # noqa: E402

TUPLES = ((), (1,), (5,), (3, 3, 3), (2, 4, 8), (8,) * 6)
C, SHAPE, SEED, NSEEDS = 5, (2, 5, 9, 11), 1234, 40
FP_FILTERS, FP_SIZE = (3, 3, 3), (128, 128)


def tuple_id(filters):
    return "f" + ("-".join(str(f) for f in filters) if filters else "none")


def perturbed(filters, dtype):
    from compressai.entropy_models import EntropyBottleneck
    eb = closed_form_fill_(EntropyBottleneck(C, filters=filters))
    eb.update(force=True)
    return eb.to(dtype)


def runs(filters, x, w, dtype):
    """every recorded tensor of one precision"""
    tag = tuple_id(filters)
    x, w = x.to(dtype), w.to(dtype)
    r = {}
    eb = perturbed(filters, dtype).train()
    eb._get_noise_cached = NoiseFeed(f"ebf:{tag}", [])
    xg = x.clone().requires_grad_(True)
    z_hat, lik = eb(xg)
    coef = -1.0 / (np.log(2.0) * x.shape[0] * x.shape[2] * x.shape[3])
    (coef * torch.log(lik).sum() + (w * z_hat).sum()).backward()
    r["train:z_hat"], r["train:lik"], r["grad:x"] = z_hat, lik, xg.grad
    for n, p in eb.named_parameters():
        if n != "quantiles":
            r[f"grad:{n}"] = p.grad
        assert (p.grad is None) == (n == "quantiles"), n
    eb.zero_grad()
    aux = eb.loss()
    aux.backward()
    r["aux"], r["aux:dq"] = aux.reshape(1), eb.quantiles.grad
    assert all(p.grad is None or n == "quantiles" or float(p.grad.abs().max()) == 0.0 for n, p in eb.named_parameters())
    eb.eval()
    with torch.no_grad():
        r["eval:z_hat"], r["eval:lik"] = eb(x)
        r["centered"] = x - eb._get_medians().detach().reshape(1, -1, 1, 1)
    return {k: t2n(v).astype(np.float64) for k, v in r.items()}


def gen_tuple(filters, d):
    from compressai.entropy_models import EntropyBottleneck
    tag = tuple_id(filters)
    torch.manual_seed(SEED)
    eb = EntropyBottleneck(C, filters=filters)
    d[f"{tag}:names"] = np.array([f"{k}|{','.join(map(str, v.shape))}" for k, v in eb.state_dict().items()])
    for n, p in eb.named_parameters():
        d[f"{tag}:init:{n}"] = t2n(p)
    w = closed_form_input(f"ebf:{tag}:w", SHAPE, -1e-3, 1e-3)
    picked = None
    for s in range(NSEEDS):
        # most of the input inside the density's support (+-10 at init_scale 10), the rest out in its tails
        x = closed_form_input(f"ebf:{tag}:x:{s}", SHAPE, -16.0, 16.0)
        r64, r32 = runs(filters, x, w, torch.float64), runs(filters, x, w, torch.float32)
        margin, dist = half_integer_margin(r64["centered"]), float(np.abs(r32["centered"] - r64["centered"]).max())
        if margin >= MARGIN_FACTOR * dist:
            picked = (s, x, r64, r32, margin, dist)
            break
    assert picked is not None, f"{tag}: no candidate input clears {MARGIN_FACTOR} x the reference's fp32 distance"
    s, x, r64, r32, margin, dist = picked
    d[f"{tag}:x"], d[f"{tag}:w"] = t2n(x), t2n(w)
    d[f"{tag}:margin"] = np.array([margin, dist, s])
    for k in r64:
        if k != "centered":
            d[f"{tag}:{k}"] = r64[k].astype(np.float32)
            d[f"{tag}:ref32:{k}"] = np.array([close_ratio(r32[k], r64[k])])
    eb = perturbed(filters, torch.float32).eval()
    for k, v in eb.state_dict().items():
        d[f"{tag}:sd:{k}"] = t2n(v)
    with torch.no_grad():
        strings = eb.compress(x)
        dec = eb.decompress(strings, x.shape[-2:])
    for b, st in enumerate(strings):
        d[f"{tag}:string:{b}"] = np.frombuffer(st, dtype=np.uint8)
    d[f"{tag}:dec"] = t2n(dec)
    assert np.array_equal(t2n(dec), r32["eval:z_hat"].astype(np.float32)), "the reference's decompress is its eval forward"
    blocked = int((r64["train:lik"] <= 1e-9).sum())
    print(f"{tag}: {len(d[f'{tag}:names'])} state-dict entries, input candidate {s}: margin {margin:.2e} ({margin / max(dist, 1e-300):.0f} x), "
          f"strings {[len(st) for st in strings]} B, {blocked} likelihoods at the floor; reference fp32 vs float64: " +
          ", ".join(f"{k} {float(d[f'{tag}:ref32:{k}'][0]):.1e}" for k in r64 if k != "centered"))


def fp_build(gain, dtype):
    from compressai.entropy_models import EntropyBottleneck
    from compressai.models.priors import FactorizedPrior
    m = FactorizedPrior(*NM)
    m.entropy_bottleneck = EntropyBottleneck(NM[1], filters=FP_FILTERS)
    m = closed_form_fill_(m).eval()
    with torch.no_grad():
        m.g_a[6].weight.mul_(gain)
        m.g_a[6].bias.mul_(gain)
        m.g_s[0].weight.mul_(G_S_SCALE / gain)
    m.update(force=True)
    return m.to(dtype)


def fp_forward(m, x):
    with torch.no_grad():
        out = m(x)
        y = m.g_a(x)
        med = m.entropy_bottleneck._get_medians().detach()
        return {k: t2n(v).astype(np.float64) for k, v in
                dict(y=y, x_hat=out["x_hat"], lik_y=out["likelihoods"]["y"], y_hat=m.entropy_bottleneck(y)[0], centered=y - med.reshape(1, -1, 1, 1)).items()}


def gen_model(d):
    picked = None
    for gain in GAINS:
        m32, m64 = fp_build(gain, torch.float32), fp_build(gain, torch.float64)
        for s in range(NSEEDS):
            seed = f"ebf:fp:{FP_SIZE[0]}x{FP_SIZE[1]}:{s}"
            x = image(seed, FP_SIZE)
            f64, f32 = fp_forward(m64, x.double()), fp_forward(m32, x)
            margin, dist = half_integer_margin(f64["centered"]), float(np.abs(f32["centered"] - f64["centered"]).max())
            if margin >= MARGIN_FACTOR * dist:
                picked = (gain, seed, x, m32, f64, f32, margin, dist)
                break
        if picked:
            break
    assert picked is not None, f"no (gain, image) candidate clears {MARGIN_FACTOR} x the reference's fp32 distance"
    gain, seed, x, m, f64, f32, margin, dist = picked
    with torch.no_grad():
        enc = m.compress(x)
        dec = m.decompress(enc["strings"], enc["shape"])
    d.update({"fp:gain": np.array([gain]), "fp:g_s_scale": np.array([G_S_SCALE / gain]), "fp:NM": np.array(NM), "fp:filters": np.array(FP_FILTERS),
              "fp:seed": np.array([seed]), "fp:size": np.array(FP_SIZE), "fp:margin": np.array([margin, dist]), "fp:shape": np.array(enc["shape"]),
              "fp:string": np.frombuffer(enc["strings"][0][0], dtype=np.uint8), "fp:x_hat": t2n(dec["x_hat"])})
    for k in ("y", "y_hat", "x_hat", "lik_y"):
        d[f"fp:fwd:{k}"] = f64[k].astype(np.float32)
        d[f"fp:ref32:{k}"] = np.array([close_ratio(f32[k], f64[k])])
    for k, v in m.entropy_bottleneck.state_dict().items():
        d[f"fp:sd:{k}"] = t2n(v)
    print(f"FactorizedPrior{NM} with filters {FP_FILTERS}: gain {gain}, {seed}: margin {margin:.2e} ({margin / max(dist, 1e-300):.0f} x), string "
          f"{len(enc['strings'][0][0])} B, y_hat non-zero {float((f64['y_hat'] != 0).mean()):.2f}; reference fp32 vs float64: " +
          ", ".join(f"{k} {float(d[f'fp:ref32:{k}'][0]):.1e}" for k in ("y", "y_hat", "x_hat", "lik_y")))


if __name__ == "__main__":
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    import_reference()
    d = {"tuples": np.array([tuple_id(f) for f in TUPLES]), "C": np.array([C]), "shape": np.array(SHAPE), "seed": np.array([SEED]),
         "margin_factor": np.array([MARGIN_FACTOR])}
    for f in TUPLES:
        gen_tuple(f, d)
    gen_model(d)
    save("eb_filters.npz", d)
