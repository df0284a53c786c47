#!/usr/bin/env python3
"""Generate the bmshj2018 fixtures from the REFERENCE itself (compressai/models/priors.py:109-313: FactorizedPrior, ScaleHyperprior;
compressai/utils/eval_model/__main__.py; the loop of compressai_examples/train.py), run as it is on the CPU.  See make_golden.py for
the import recipe this builds on, make_golden_cheng.py for the margin rule.

    python tests/golden/make_golden_bmshj.py

  bmshj_names.npz           ordered state-dict keys with shapes of both classes at (N, M) = (128, 192) and (192, 320)
  bmshj_codec.<m>.npz       <m> = factorized | hyperprior: the class at (64, 96), closed_form_fill_, the last analysis convolution x gain
                            and the first synthesis convolution x 0.25 / gain (build); one 128 x 128 and one 128 x 192 image: compress
                            strings, shape, decompress x_hat, the eval forward in float64 with the fp32 run's distance per tensor
                            (conftest.close_ratio, floor 0.1), the CDF tables, and the MARGINS below
  bmshj_train.npz           both classes at (64, 96), batch 2 of 128 x 128, noise fed by name (make_golden.NoiseFeed):
                            RateDistortionLoss(lmbda=1e-2) terms, aux_loss, and digests of the gradient of every parameter and of the
                            input -- (sum, sum |.|, sum of squares, count) and a strided slice, the tensors themselves are megabytes --
                            then the same digests of the parameters, and of their change, after two steps of train.py's loop
                            (Adam 1e-4, aux Adam 1e-3, clip 1.0).  All float64, with the fp32 run's distance per tensor.
  bmshj_image_eval.npz      eval_model's `inference` on one 120 x 104 image per model (padded to 128 x 128 there), and its
                            `inference_entropy_estimation` on one 128 x 128 image: at 120 x 104 that function raises in the reference
                            (it does not pad, and the strides do not divide the sides).  bpp and psnr; ms-ssim is dropped, as in
                            eval_gop.npz (the package is not in the reference tree).

Margins.  Byte identity is a fair demand only where no symbol sits on a threshold, so the codec fixture is CHOSEN: candidates
(gain, image seed) are tried in a fixed order and the first is kept whose margins, computed from the eval forward, are all at least
MARGIN_FACTOR x the reference's own fp32-vs-float64 distance (largest element) on the tensor concerned:
    factorized:  y - median from a half-integer (the only threshold: the bottleneck's rounding)
    hyperprior:  y from a half-integer, z - median from a half-integer, scales_hat from a scale-table entry (relative)
The factorized model MUST clear the factor (asserted here).  For the hyper-prior model the scale-table margin falls under
make_golden_cheng.py's rule: where no candidate clears the factor the best one is kept and `margins_cleared` = 0 says so.
Float64 tensors are stored rounded to float32; images are regenerated from their seed names, not stored.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import NoiseFeed, closed_form_fill_, import_reference, save, smooth_frames, t2n  # noqa: E402
from make_golden_cheng import MARGIN_FACTOR, close_ratio, half_integer_margin, image  # noqa: E402

GAINS = (4.0, 2.0, 1.0, 0.5, 0.25)
NSEEDS = 40
G_S_SCALE = 0.25
SIZES = ((128, 128), (128, 192))
NM = (64, 96)
EVAL_SIZE = (120, 104)
TAGS = ("factorized", "hyperprior")
SLICE = 64
LMBDA, LR, AUX_LR, CLIP = 1e-2, 1e-4, 1e-3, 1.0
TABLE_KEYS = {"factorized": ("entropy_bottleneck._quantized_cdf", "entropy_bottleneck._offset", "entropy_bottleneck._cdf_length"),
              "hyperprior": ("entropy_bottleneck._quantized_cdf", "entropy_bottleneck._offset", "entropy_bottleneck._cdf_length",
                             "gaussian_conditional._quantized_cdf", "gaussian_conditional._offset", "gaussian_conditional._cdf_length")}


def classes():
    from compressai.models.priors import FactorizedPrior, ScaleHyperprior
    return {"factorized": FactorizedPrior, "hyperprior": ScaleHyperprior}


def build(cls, gain):
    """closed_form_fill_, the last analysis convolution x gain (so that the symbols are neither all zero nor huge) and the first
    synthesis convolution x G_S_SCALE / gain (make_golden.eval_gop_models' x4, x1/4): with the plain fill the three inverse GDNs take
    the image to +-20; at 0.25 it stays within +-2, about half of the decoded pixels strictly inside (0, 1)"""
    m = closed_form_fill_(cls(*NM)).eval()
    with torch.no_grad():
        m.g_a[6].weight.mul_(gain)
        m.g_a[6].bias.mul_(gain)
        m.g_s[0].weight.mul_(G_S_SCALE / gain)
    m.update(force=True)
    return m


def gen_names():
    d = {}
    for tag, cls in classes().items():
        for N, M in ((128, 192), (192, 320)):
            d[f"{tag}:{N},{M}"] = np.array([f"{k}|{','.join(map(str, v.shape))}" for k, v in cls(N, M).state_dict().items()])
    save("bmshj_names.npz", d)


def eval_forward(m, x, tag):
    with torch.no_grad():
        out = m(x)
        y = m.g_a(x)
        med = m.entropy_bottleneck._get_medians().detach()
        res = {"y": y, "x_hat": out["x_hat"], "lik_y": out["likelihoods"]["y"]}
        if tag == "factorized":
            res["y_hat"] = m.entropy_bottleneck(y)[0]
            res["y_centered"] = y - med.reshape(1, -1, 1, 1)
        else:
            z = m.h_a(torch.abs(y))
            res.update(y_hat=torch.round(y), lik_z=out["likelihoods"]["z"], scales=m.h_s(m.entropy_bottleneck(z)[0]),
                       z_centered=z - med.reshape(1, -1, 1, 1))
    return res


FWD_KEYS = {"factorized": ("y", "y_hat", "x_hat", "lik_y"), "hyperprior": ("y", "y_hat", "x_hat", "lik_y", "lik_z", "scales")}


def margins(m32, m64, x, tag):
    """-> (float64 forward, fp32 forward, {name: (margin, reference-fp32 distance)})"""
    f32 = {k: t2n(v) for k, v in eval_forward(m32, x, tag).items()}
    f64 = {k: t2n(v) for k, v in eval_forward(m64, x.double(), tag).items()}
    if tag == "factorized":
        return f64, f32, {"y_minus_median": (half_integer_margin(f64["y_centered"]), float(np.abs(f32["y_centered"] - f64["y_centered"]).max()))}
    table = t2n(m64.gaussian_conditional.scale_table).astype(np.float64)
    return f64, f32, {"y": (half_integer_margin(f64["y"]), float(np.abs(f32["y"] - f64["y"]).max())),
                      "z_minus_median": (half_integer_margin(f64["z_centered"]), float(np.abs(f32["z_centered"] - f64["z_centered"]).max())),
                      "scales_rel": (float((np.abs(f64["scales"][..., None] - table) / table).min()),
                                     float((np.abs(f32["scales"] - f64["scales"]) / np.maximum(np.abs(f64["scales"]), table[0])).max()))}


def choose(cls, tag):
    """make_golden_cheng.choose: -> (gain, model, [(seed, size, f64, f32, margins)], cleared)"""
    best = None
    for gain in GAINS:
        m32, m64 = build(cls, gain), build(cls, gain).double()
        picked, cleared = [], True
        for size in SIZES:
            top = None
            for s in range(NSEEDS):
                seed = f"bmshj:{tag}:{size[0]}x{size[1]}:{s}"
                f64, f32, res = margins(m32, m64, image(seed, size), tag)
                ratio = min(mg / max(dist, 1e-300) for mg, dist in res.values())
                if top is None or ratio > top[0]:
                    top = (ratio, (seed, size, f64, f32, res))
                if ratio >= MARGIN_FACTOR:
                    break
            cleared &= top[0] >= MARGIN_FACTOR
            picked.append(top)
        worst = min(t[0] for t in picked)
        print(f"  {tag}: gain {gain}: worst margin / distance ratio {worst:.1f} ({', '.join(t[1][0] for t in picked)})")
        if cleared:
            return gain, m32, [t[1] for t in picked], True
        if best is None or worst > best[0]:
            best = (worst, gain, [t[1] for t in picked])
    print(f"  {tag}: NO candidate clears {MARGIN_FACTOR:.0f} x; keeping gain {best[1]} with a worst ratio of {best[0]:.1f}")
    return best[1], build(cls, best[1]), best[2], False


def gen_codec():
    chosen = {}
    for tag, cls in classes().items():
        gain, m, picked, cleared = choose(cls, tag)
        assert cleared or tag != "factorized", "the factorized model's only threshold must clear the margin factor"
        chosen[tag] = gain
        d = {"gain": np.array([gain]), "g_s_scale": np.array([G_S_SCALE / gain]), "NM": np.array(NM), "margin_factor": np.array([MARGIN_FACTOR]), "margins_cleared": np.array([int(cleared)]),
             "seeds": np.array([p[0] for p in picked]), "sizes": np.array([p[1] for p in picked])}
        for i, (seed, size, f64, f32, res) in enumerate(picked):
            x = image(seed, size)
            with torch.no_grad():
                enc = m.compress(x)
                dec = m.decompress(enc["strings"], enc["shape"])
            for name, s in zip(("y_string", "z_string"), enc["strings"]):
                d[f"{i}:{name}"] = np.frombuffer(s[0], dtype=np.uint8)
            d[f"{i}:shape"] = np.array(enc["shape"])
            d[f"{i}:x_hat"] = t2n(dec["x_hat"])
            for k in FWD_KEYS[tag]:
                d[f"{i}:fwd:{k}"] = f64[k].astype(np.float32)
                d[f"{i}:ref32:{k}"] = np.array([close_ratio(f32[k], f64[k])])
            d[f"{i}:margin_names"] = np.array(list(res))
            d[f"{i}:margins"] = np.array([v[0] for v in res.values()])
            d[f"{i}:margin_ref32"] = np.array([v[1] for v in res.values()])
            inside = float(((dec["x_hat"] > 0) & (dec["x_hat"] < 1)).float().mean())
            print(f"{tag} gain {gain} {seed}: strings {[len(s[0]) for s in enc['strings']]} B, y_hat non-zero {float((f64['y_hat'] != 0).mean()):.2f}, "
                  f"|y| max {np.abs(f64['y']).max():.2f}, decoded pixels strictly inside (0, 1): {inside:.2f}")
            for k, (mg, dist) in res.items():
                print(f"    margin {k}: {mg:.3e}   reference fp32 vs float64: {dist:.3e}   ratio {mg / max(dist, 1e-300):.0f}")
            print("    reference fp32 vs float64 (close_ratio, floor 0.1): " + ", ".join(f"{k} {float(d[f'{i}:ref32:{k}'][0]):.1e}" for k in FWD_KEYS[tag]))
        sd = m.state_dict()
        for k in TABLE_KEYS[tag]:
            d[k] = t2n(sd[k]).astype(np.int32)
        if tag == "hyperprior":
            d["gaussian_conditional.scale_table"] = t2n(sd["gaussian_conditional.scale_table"])
        save(f"bmshj_codec.{tag}.npz", d)
    return chosen


# ---- training ---------------------------------------------------------------------------------------------------------------
def digest(t):
    """(sum, sum |.|, sum of squares, count) and a strided slice of at most SLICE elements, both float64"""
    t = t.detach().double().reshape(-1)
    return (np.array([float(t.sum()), float(t.abs().sum()), float((t * t).sum()), float(t.numel())]),
            t2n(t[:: max(1, t.numel() // SLICE)][:SLICE]))


def rd_loss(out, target):
    """the reference's RateDistortionLoss (utils.py:30-50) at lmbda = LMBDA, in the tensors' own precision"""
    n, _, h, w = target.shape
    bpp = sum(torch.log(lik).sum() / (-np.log(2) * n * h * w) for lik in out["likelihoods"].values())
    mse = torch.nn.functional.mse_loss(out["x_hat"], target)
    return {"bpp_loss": bpp, "mse_loss": mse, "loss": LMBDA * 255 ** 2 * mse + bpp}


def train_model(cls, tag, role, dtype):
    m = closed_form_fill_(cls(*NM)).to(dtype).train()
    log = []
    m.entropy_bottleneck._get_noise_cached = NoiseFeed(f"bmshj:{tag}:{role}_eb", log)
    if tag == "hyperprior":
        m.gaussian_conditional._get_noise_cached = NoiseFeed(f"bmshj:{tag}:{role}_gc", log)
    return m


def train_runs(cls, tag, dtype):
    """-> {key: (sums, slice)} and {scalar name: value} of one precision"""
    x = smooth_frames(f"bmshj:{tag}:train", 2, 1, 128)[0].to(dtype)
    res, scal = {}, {}
    # (a) one training pass: loss terms, aux loss, every gradient
    m = train_model(cls, tag, "grad", dtype)
    xg = x.clone().requires_grad_(True)
    oc = rd_loss(m(xg), x)
    oc["loss"].backward()
    scal.update({k: float(v) for k, v in oc.items()}, aux_loss=float(m.aux_loss()))
    res["d:x"] = digest(xg.grad)
    for n, p in m.named_parameters():
        if p.grad is not None:
            res[f"d:{n}"] = digest(p.grad)
    # (b) two steps of compressai_examples/train.py:127-143
    m = train_model(cls, tag, "step", dtype)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    params = dict(m.named_parameters())
    opt = torch.optim.Adam([params[n] for n in sorted(params) if not n.endswith(".quantiles")], lr=LR)
    aux = torch.optim.Adam([params[n] for n in sorted(params) if n.endswith(".quantiles")], lr=AUX_LR)
    for step in range(2):
        opt.zero_grad()
        aux.zero_grad()
        oc = rd_loss(m(x), x)
        oc["loss"].backward()
        norm = torch.nn.utils.clip_grad_norm_(m.parameters(), CLIP)
        opt.step()
        a = m.aux_loss()
        a.backward()
        aux.step()
        scal.update({f"step{step}:loss": float(oc["loss"]), f"step{step}:aux_loss": float(a), f"step{step}:grad_norm": float(norm)})
    for n, p in m.named_parameters():
        res[f"p:{n}"] = digest(p)
        res[f"delta:{n}"] = digest(p.detach() - before[n])
    return res, scal


def gen_train():
    d = {"NM": np.array(NM), "hyper": np.array([LMBDA, LR, AUX_LR, CLIP]), "slice": np.array([SLICE])}
    for tag, cls in classes().items():
        r64, s64 = train_runs(cls, tag, torch.float64)
        r32, s32 = train_runs(cls, tag, torch.float32)
        d[f"{tag}:scalar_names"] = np.array(list(s64))
        d[f"{tag}:scalars"] = np.array([s64[k] for k in s64])
        d[f"{tag}:scalars_ref32"] = np.array([abs(s32[k] - s64[k]) / max(abs(s64[k]), 1e-300) for k in s64])
        d[f"{tag}:keys"] = np.array(list(r64))
        worst = {}
        for k, (sums, sl) in r64.items():
            d[f"{tag}:sum:{k}"], d[f"{tag}:slice:{k}"] = sums, sl
            rms = float(np.sqrt(sums[2] / sums[3]))
            # the slice against float64, relative to the element or 0.1 x the slice's maximum; the sums relative to sum |.|
            d[f"{tag}:ref32:{k}"] = np.array([close_ratio(r32[k][1], sl) if np.abs(sl).max() > 0 else 0.0,
                                              float(np.abs(r32[k][0][:2] - sums[:2]).max() / max(sums[1], 1e-300)), rms])
            kind = k.split(":", 1)[0]
            worst[kind] = max(worst.get(kind, 0.0), float(d[f"{tag}:ref32:{k}"][0]))
        print(f"train {tag}: " + ", ".join(f"{k} {v:.6g}" for k, v in s64.items()))
        print(f"    {len(r64)} digests; reference fp32 vs float64 at most " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    save("bmshj_train.npz", d)


# ---- eval_model ---------------------------------------------------------------------------------------------------------------
def import_eval_model(scratch):
    """compressai/utils/eval_model/__main__.py as a module.  It imports pytorch_msssim, which this image does not have and whose
    number is not recorded: a stand-in returning zero is put on the scratch path, as make_golden._import_reference_eval_script does."""
    os.makedirs(os.path.join(scratch, "pytorch_msssim"), exist_ok=True)
    with open(os.path.join(scratch, "pytorch_msssim", "__init__.py"), "w") as f:
        f.write("import torch\ndef ms_ssim(*a, **k):\n    return torch.zeros(())\n")
    spec = importlib.util.spec_from_file_location("ref_eval_model", os.path.join(scratch, "compressai", "utils", "eval_model", "__main__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gen_image_eval(scratch, gains):
    ev = import_eval_model(scratch)
    h, w = EVAL_SIZE
    d = {"size": np.array([h, w]), "NM": np.array(NM), "est_size": np.array([128, 128])}
    for tag, cls in classes().items():
        m = build(cls, gains[tag])
        x = smooth_frames(f"bmshj:{tag}:eval", 1, 1, 128)[0][0, :, 4:4 + h, 12:12 + w].contiguous()
        xe = smooth_frames(f"bmshj:{tag}:eval", 1, 1, 128)[0][0].contiguous()
        try:
            ev.inference_entropy_estimation(m, x)
            raise AssertionError("inference_entropy_estimation ran on an unpadded 120 x 104 image: record it at that size")
        except RuntimeError:
            pass
        coded, est = ev.inference(m, x), ev.inference_entropy_estimation(m, xe)
        d[f"{tag}:gain"], d[f"{tag}:g_s_scale"] = np.array([gains[tag]]), np.array([G_S_SCALE / gains[tag]])
        d[f"{tag}:coded"] = np.array([coded["bpp"], coded["psnr"]], dtype=np.float64)
        d[f"{tag}:estimate"] = np.array([est["bpp"], est["psnr"]], dtype=np.float64)
        sd = m.state_dict()
        for k in TABLE_KEYS[tag]:
            d[f"{tag}:{k}"] = t2n(sd[k]).astype(np.int32)
        print(f"eval_model {tag}: coded bpp {coded['bpp']:.4f} PSNR {coded['psnr']:.3f} dB; estimate (128 x 128) bpp {est['bpp']:.4f} PSNR {est['psnr']:.3f} dB")
    save("bmshj_image_eval.npz", d)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    scratch, _ = import_reference()
    gen_names()
    gains = gen_codec()
    gen_train()
    gen_image_eval(scratch, gains)
