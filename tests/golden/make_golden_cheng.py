#!/usr/bin/env python3
"""Generate the cheng2020 fixtures from the REFERENCE itself (compressai/models/waseda.py, compressai/layers/layers.py:50-213,
stem/evalSTEM.py), run as it is on the CPU.  See make_golden.py for the import recipe this builds on.

    python tests/golden/make_golden_cheng.py

  cheng_names.npz         ordered state-dict keys with shapes of Cheng2020Anchor / Cheng2020Attention at N = 128 and N = 192
  cheng_blocks.npz        the four block types at small widths on closed_form_fill_ weights, input 2 x C x 6 x 10: the float64 output,
                          the float64 gradients of a fixed cotangent with respect to the input and every parameter, and per tensor the
                          distance of the reference's own fp32 run from that float64 run (conftest.close_ratio, floor 0.1)
  cheng_codec.<m>.npz     <m> = anchor | attn: Cheng2020Anchor(64) / Cheng2020Attention(64), closed_form_fill_, the last analysis
                          convolution x gain, the synthesis convolutions x 0.5 (build); one 128 x 128 and one 128 x 192 image: compress strings, shape, decompress x_hat / y_hat,
                          the eval forward in float64 with the fp32 run's distance per tensor, the CDF tables, and the MARGINS below
  cheng_gop.npz           stem/evalSTEM.py's inferenceI_DVR / inferenceP_DVR on one I and two P frames, Cheng2020Anchor(96) in front of
                          the small SpatioTemporalPriorModel_Res(64, 96): every string, shape, bpp, estimate_bpp, PSNR

Margins.  Byte identity is a fair demand only where no symbol sits on a threshold, so the codec fixture is CHOSEN: candidates
(gain, image seed) are tried in a fixed order and the first is kept whose margins, computed from the eval forward, are all at
least MARGIN_FACTOR x the reference's own fp32-vs-float64 distance (largest element) on the tensor concerned:
    y - means_hat from a half-integer (the coder's rounding),   y from a half-integer (forward's y_hat = round(y)),
    z - median from a half-integer,   scales_hat from a scale-table entry (relative).
Margins, distances and the chosen candidate are stored and printed.  Where NO candidate clears the factor the one with the
largest worst ratio is kept and the fixture says so (`margins_cleared` = 0): with these weights about a third of the scales lie
inside the table's range, entries 13 % apart, against an fp32 distance of 1e-5 of a scale -- thousands of elements all
5e-4 away from an entry is not something a search over seeds finds.  Float64 tensors are stored rounded to float32 (2^-24 of
their value, against gates of 1e-4) to keep the files small; images are regenerated from their seed names, not stored.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import (  # noqa: E402
    _import_reference_eval_script,
    closed_form_fill_,
    closed_form_input,
    import_reference,
    save,
    smooth_frames,
    t2n,
)

MARGIN_FACTOR = 50.0
GAINS = (4.0, 1.0, 0.25, 0.125, 0.06, 0.03)
NSEEDS = 40
G_S_SCALE = 0.5
SIZES = ((128, 128), (128, 192))
GOP_SIZE = (120, 104)               # as make_golden.EVAL_GOP_SIZE: padded to 128 x 128 by the script


def close_ratio(a, b, floor=0.1):
    """tests/conftest.py:close_ratio"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.abs(b).max()), 1e-30)
    return float((np.abs(a - b) / np.maximum(np.abs(b), floor * scale)).max())


def image(seed, size):
    """[1, 3, h, w] in [0, 1]: the top rows of a square smooth frame whose side is the width"""
    h, w = size
    return smooth_frames(seed, 1, 1, max(h, w))[0][:, :, :h, :w].contiguous()


def last_analysis_conv(m):
    convs = [c for c in m.g_a.children() if isinstance(c, torch.nn.Conv2d)]
    assert len(convs) == 1
    return convs[0]


def build(cls, N, gain):
    """closed_form_fill_, the last analysis convolution x gain (so that the symbols are neither all zero nor huge) and every
    convolution weight of g_s x G_S_SCALE: with the plain fill the three inverse GDNs behind residual sums take the image to 1e2
    (anchor) .. 1e8 (attention); at 0.5 it stays of order one, about half of the decoded pixels strictly inside (0, 1).  The
    counterpart of gen_iframe_codec's x4 / x1/4."""
    m = closed_form_fill_(cls(N)).eval()
    with torch.no_grad():
        c = last_analysis_conv(m)
        c.weight.mul_(gain)
        c.bias.mul_(gain)
        for p in m.g_s.parameters():
            if p.dim() == 4:
                p.mul_(G_S_SCALE)
    m.update(force=True)
    return m


def gen_names():
    from compressai.models.waseda import Cheng2020Anchor, Cheng2020Attention
    d = {}
    for tag, cls in (("anchor", Cheng2020Anchor), ("attn", Cheng2020Attention)):
        for N in (128, 192):
            d[f"{tag}:{N}"] = np.array([f"{k}|{','.join(map(str, v.shape))}" for k, v in cls(N).state_dict().items()])
    save("cheng_names.npz", d)


def gen_blocks():
    from compressai.layers import AttentionBlock, ResidualBlock, ResidualBlockUpsample, ResidualBlockWithStride
    cases = (("rbs_3_32", lambda: ResidualBlockWithStride(3, 32), 3), ("rbs_32_32", lambda: ResidualBlockWithStride(32, 32), 32),
             ("rb_32_32", lambda: ResidualBlock(32, 32), 32), ("rbu_32_32", lambda: ResidualBlockUpsample(32, 32, 2), 32),
             ("attn_32", lambda: AttentionBlock(32), 32), ("attn_24", lambda: AttentionBlock(24), 24))
    d = {"cases": np.array([c[0] for c in cases])}
    for tag, make, cin in cases:
        runs = {}
        for dtype in (torch.float64, torch.float32):
            blk = closed_form_fill_(make()).to(dtype)
            x = closed_form_input(f"cheng:{tag}:x", (2, cin, 6, 10), 0.0 if cin == 3 else -1.0, 1.0).to(dtype).requires_grad_(True)
            out = blk(x)
            g = closed_form_input(f"cheng:{tag}:g", tuple(out.shape), -1.0, 1.0).to(dtype)
            out.backward(g)
            runs[dtype] = {"out": t2n(out), "dx": t2n(x.grad), **{f"d:{n}": t2n(p.grad) for n, p in blk.named_parameters()}}
        d[f"{tag}:params"] = np.array([k[2:] for k in runs[torch.float64] if k.startswith("d:")])
        worst = 0.0
        for k, v in runs[torch.float64].items():
            d[f"{tag}:{k}"] = v.astype(np.float32)
            d[f"{tag}:ref32:{k}"] = np.array([close_ratio(runs[torch.float32][k], v)])
            worst = max(worst, float(d[f"{tag}:ref32:{k}"][0]))
        print(f"block {tag}: out {tuple(runs[torch.float64]['out'].shape)}, {len(runs[torch.float64]) - 2} parameter gradients, "
              f"reference-fp32 vs float64 at most {worst:.2e}")
    save("cheng_blocks.npz", d)


def half_integer_margin(v):
    v = np.asarray(v, np.float64)
    return float(np.abs(v - np.floor(v) - 0.5).min())


def eval_forward(m, x):
    with torch.no_grad():
        out = m(x)
        z = m.h_a(out["y"])
        med = m.entropy_bottleneck._get_medians().detach()
    return {"y": out["y"], "y_hat": out["y_hat"], "x_hat": out["x_hat"], "lik_y": out["likelihoods"]["y"], "lik_z": out["likelihoods"]["z"],
            "scales": out["entropy_params"]["scales_hat"], "means": out["entropy_params"]["means_hat"], "z": z, "z_centered": z - med}


def margins(m32, m64, x):
    """-> (float64 forward, fp32 forward, {name: (margin, reference-fp32 distance)})"""
    f32 = {k: t2n(v) for k, v in eval_forward(m32, x).items()}
    f64 = {k: t2n(v) for k, v in eval_forward(m64, x.double()).items()}
    table = t2n(m64.gaussian_conditional.scale_table).astype(np.float64)
    res = {"y_minus_means": (half_integer_margin(f64["y"] - f64["means"]), float(np.abs((f32["y"] - f32["means"]) - (f64["y"] - f64["means"])).max())),
           "y": (half_integer_margin(f64["y"]), float(np.abs(f32["y"] - f64["y"]).max())),
           "z_minus_median": (half_integer_margin(f64["z_centered"]), float(np.abs(f32["z_centered"] - f64["z_centered"]).max())),
           "scales_rel": (float((np.abs(f64["scales"][..., None] - table) / table).min()),
                          float((np.abs(f32["scales"] - f64["scales"]) / np.maximum(np.abs(f64["scales"]), table[0])).max()))}
    return f64, f32, res


def choose(cls, tag):
    """-> (gain, model, [(seed, size, f64, f32, margins)], cleared).  The first gain for which both image sizes have a seed whose
    margins clear MARGIN_FACTOR x the fp32 distance (per size: the first such seed).  Where no gain has one, the candidates
    with the largest worst margin / distance ratio are kept instead (per gain and size the best seed, then the best gain),
    `cleared` is False and the ratios say by how much the factor was missed."""
    best = None
    for gain in GAINS:
        m32 = build(cls, 64, gain)
        m64 = build(cls, 64, gain).double()              # (the coder objects inside an updated model cannot be deep-copied)
        picked, cleared = [], True
        for size in SIZES:
            top = None
            for s in range(NSEEDS):
                seed = f"cheng:{tag}:{size[0]}x{size[1]}:{s}"
                f64, f32, res = margins(m32, m64, image(seed, size))
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
    return best[1], build(cls, 64, best[1]), best[2], False


def gen_codec():
    from compressai.models.waseda import Cheng2020Anchor, Cheng2020Attention
    chosen_gain = {}
    for tag, cls in (("anchor", Cheng2020Anchor), ("attn", Cheng2020Attention)):
        gain, m, picked, cleared = choose(cls, tag)
        chosen_gain[tag] = gain
        d = {"gain": np.array([gain]), "g_s_scale": np.array([G_S_SCALE]), "N": np.array([64]), "margin_factor": np.array([MARGIN_FACTOR]), "margins_cleared": np.array([int(cleared)]),
             "seeds": np.array([p[0] for p in picked]), "sizes": np.array([p[1] for p in picked])}
        for i, (seed, size, f64, f32, res) in enumerate(picked):
            x = image(seed, size)
            with torch.no_grad():
                enc = m.compress(x)
                dec = m.decompress(enc["strings"], enc["shape"])
            d[f"{i}:y_string"] = np.frombuffer(enc["strings"][0][0], dtype=np.uint8)
            d[f"{i}:z_string"] = np.frombuffer(enc["strings"][1][0], dtype=np.uint8)
            d[f"{i}:shape"] = np.array(enc["shape"])
            d[f"{i}:x_hat"], d[f"{i}:y_hat"] = t2n(dec["x_hat"]), t2n(dec["y_hat"])
            for k in ("y", "y_hat", "x_hat", "lik_y", "lik_z", "scales", "means"):
                d[f"{i}:fwd:{k}"] = f64[k].astype(np.float32)
                d[f"{i}:ref32:{k}"] = np.array([close_ratio(f32[k], f64[k])])
            d[f"{i}:margin_names"] = np.array(list(res))
            d[f"{i}:margins"] = np.array([v[0] for v in res.values()])
            d[f"{i}:margin_ref32"] = np.array([v[1] for v in res.values()])
            nz = float((t2n(dec["y_hat"]) != 0).mean())
            inside = float(((dec["x_hat"] > 0) & (dec["x_hat"] < 1)).float().mean())
            print(f"{tag} gain {gain} {seed}: y {len(enc['strings'][0][0])} B, z {len(enc['strings'][1][0])} B, y_hat non-zero {nz:.2f}, "
                  f"|y| max {np.abs(f64['y']).max():.2f}, decoded pixels strictly inside (0, 1): {inside:.2f}")
            for k, (mg, dist) in res.items():
                print(f"    margin {k}: {mg:.3e}   reference fp32 vs float64: {dist:.3e}   ratio {mg / max(dist, 1e-300):.0f}")
            print("    reference fp32 vs float64 (close_ratio, floor 0.1): " +
                  ", ".join(f"{k} {float(d[f'{i}:ref32:{k}'][0]):.1e}" for k in ("y", "x_hat", "lik_y", "lik_z", "scales", "means")))
        sd = m.state_dict()
        for k in ("entropy_bottleneck._quantized_cdf", "entropy_bottleneck._offset", "entropy_bottleneck._cdf_length",
                  "gaussian_conditional._quantized_cdf", "gaussian_conditional._offset", "gaussian_conditional._cdf_length"):
            d[k] = t2n(sd[k]).astype(np.int32)
        d["gaussian_conditional.scale_table"] = t2n(sd["gaussian_conditional.scale_table"])
        save(f"cheng_codec.{tag}.npz", d)
    return chosen_gain


def gen_gop(scratch, gain, nframes=3):
    from compressai.models.spatiotemporalpriors import SpatioTemporalPriorModel_Res
    from compressai.models.waseda import Cheng2020Anchor
    ev = _import_reference_eval_script(scratch)
    imodel = build(Cheng2020Anchor, 96, gain)
    stem = closed_form_fill_(SpatioTemporalPriorModel_Res(64, 96)).eval()
    stem.update(force=True)
    h, w = GOP_SIZE
    frames = [f[0, :, 4:4 + h, 12:12 + w].contiguous() for f in smooth_frames("cheng:gop", 1, nframes, 128)]
    d = {"size": np.array([h, w]), "nframes": np.array([nframes]), "gain": np.array([gain]), "g_s_scale": np.array([G_S_SCALE]), "N": np.array([96])}
    captured = {}

    def tap(model, name):
        real = model.compress

        def compress(*a, **k):
            out = real(*a, **k)
            captured[name] = out
            return out
        model.compress = compress

    tap(imodel, "i"), tap(stem, "p")
    real_decompress = stem.decompress                          # see make_golden.gen_eval_gop: the key the script reads last
    stem.decompress = lambda *a, **k: dict(real_decompress(*a, **k), entropy_params=None)
    with contextlib.redirect_stdout(io.StringIO()):
        out = ev.inferenceI_DVR(imodel, frames[0])
    y_cond = out["y_conditioned"]
    for t in range(nframes):
        if t > 0:
            with contextlib.redirect_stdout(io.StringIO()):
                out = ev.inferenceP_DVR(imodel, stem, frames[t], y_cond)
            y_cond = out["y_conditioned"]
        enc = captured["i" if t == 0 else "p"]
        d[f"f{t}:y_string"] = np.frombuffer(enc["strings"][0][0], dtype=np.uint8)
        d[f"f{t}:z_string"] = np.frombuffer(enc["strings"][1][0], dtype=np.uint8)
        d[f"f{t}:shape"] = np.array(enc["shape"])
        d[f"f{t}:scalars"] = np.array([out["bpp"], out["estimate_bpp"], out["psnr"]], dtype=np.float64)
        d[f"f{t}:y_conditioned"] = t2n(y_cond)
        print(f"cheng gop frame {t}: y {len(enc['strings'][0][0])} B, z {len(enc['strings'][1][0])} B, bpp {out['bpp']:.4f} "
              f"(estimate {out['estimate_bpp']:.4f}), PSNR {out['psnr']:.3f} dB")
    with torch.no_grad():
        d["last:x_hat"] = t2n(imodel.getX(y_cond)[:, :, 4:4 + h, 12:12 + w])
    for tag, m in (("i", imodel), ("p", stem)):
        d[f"{tag}:eb_cdf"], d[f"{tag}:eb_offset"] = t2n(m.entropy_bottleneck._quantized_cdf), t2n(m.entropy_bottleneck._offset)
        d[f"{tag}:eb_cdf_length"] = t2n(m.entropy_bottleneck._cdf_length)
        d[f"{tag}:gc_cdf"] = t2n(m.gaussian_conditional._quantized_cdf).astype(np.int32)
        d[f"{tag}:gc_offset"], d[f"{tag}:gc_cdf_length"] = t2n(m.gaussian_conditional._offset), t2n(m.gaussian_conditional._cdf_length)
    save("cheng_gop.npz", d)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    scratch, _ = import_reference()
    gen_names()
    gen_blocks()
    gains = gen_codec()
    gen_gop(scratch, gains["anchor"])
