#!/usr/bin/env python3
"""Generate tests/golden/pixel_eval_roi.npz and tests/golden/pixel_eval_baseline.npz from the REFERENCE itself: the evaluation
functions of stem_roi/eval_stem_roi.py and stem_roi/eval_stem_baseline.py, imported as modules and run as they are.

Run by hand on the CPU, where the reference tree is (see make_golden.py for the import recipe this builds on):

    python tests/golden/make_golden_pixel_eval.py

Two chains of three frames (I, P, P) of 104 x 72 pixels -- padded by the scripts to 128 x 128 with 12 rows above / below and 28
columns left / right -- with the scripts' feedback (the next frame is conditioned on the cropped x_hat of this one):

    roi       stem_roi_i + stem_roi, closed_form_fill_scaled_("roi_i" / "roi_p", 0.7), one non-uniform quality map
    baseline  MeanScaleHyperprior(64, 96) + stem_baseline (eval_stem_baseline.py:294-297 pairs them)

Recorded per frame: the byte counts of both strings, `shape`, bpp / estimate_bpp / PSNR and the cropped x_hat; per model the CDF
tables (they travel with a checkpoint).  For MeanScaleHyperprior also one training-mode forward with injected noise and the
state-dict key list with shapes.  Only inputs and outputs are saved.
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import (  # noqa: E402
    REF,
    NoiseFeed,
    _import_reference_eval_script,
    closed_form_fill_scaled_,
    closed_form_input,
    import_reference,
    save,
    smooth_frames,
    t2n,
)

SIZE = (104, 72)                    # h, w: neither a multiple of 64
TOP, LEFT = 12, 28                  # the borders of the centred 128 x 128 padding
ROI_CONV_SCALE = 0.7


def _import_script(scratch, name):
    """stem_roi/<name>.py as a module.  Stand-ins for what the scripts import and their inference functions never use (cv2) or use
    for a number that is not recorded (pytorch_msssim, through make_golden._import_reference_eval_script's scheme)."""
    _import_reference_eval_script(scratch)                      # puts the pytorch_msssim stand-in on the scratch path
    os.makedirs(os.path.join(scratch, "cv2"), exist_ok=True)
    open(os.path.join(scratch, "cv2", "__init__.py"), "w").close()
    keep = os.environ.get("CUDA_VISIBLE_DEVICES")
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "stem_roi", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                # (sets CUDA_VISIBLE_DEVICES at import: restored)
    if keep is None:
        os.environ.pop("CUDA_VISIBLE_DEVICES", None)
    else:
        os.environ["CUDA_VISIBLE_DEVICES"] = keep
    return mod


def frames3():
    h, w = SIZE
    return [f[:, :, TOP:TOP + h, LEFT:LEFT + w].contiguous() for f in smooth_frames("pixeleval", 1, 3, 128)]


def _tap(model, captured, name):
    real = model.compress

    def compress(*a, **k):
        out = real(*a, **k)
        captured[name] = out
        return out
    model.compress = compress


def _tables(d, tag, m):
    sd = m.state_dict()
    for k in ("entropy_bottleneck._quantized_cdf", "entropy_bottleneck._offset", "entropy_bottleneck._cdf_length",
              "gaussian_conditional._quantized_cdf", "gaussian_conditional._offset", "gaussian_conditional._cdf_length"):
        d[f"{tag}:{k}"] = t2n(sd[k]).astype(np.int32)


def _chain(d, model_i, model_p, run_i, run_p):
    """the scripts' loop (eval_stem_roi.py:237-242) over the three frames; records what each call returns"""
    captured = {}
    _tap(model_i, captured, "i"), _tap(model_p, captured, "p")
    x_cond = None
    for t, x in enumerate(frames3()):
        with contextlib.redirect_stdout(io.StringIO()):
            out = run_i(x) if t == 0 else run_p(x, x_cond)
        x_cond = out["x_hat"]
        enc = captured["i" if t == 0 else "p"]
        d[f"f{t}:nbytes"] = np.array([len(enc["strings"][0][0]), len(enc["strings"][1][0])])
        d[f"f{t}:shape"] = np.array(enc["shape"])
        d[f"f{t}:scalars"] = np.array([out["bpp"], out["estimate_bpp"], out["psnr"]], dtype=np.float64)
        d[f"f{t}:x_hat"] = t2n(out["x_hat"])
        y = enc["strings"][0][0]
        print(f"  frame {t}: y {len(y)} B, z {len(enc['strings'][1][0])} B, bpp {out['bpp']:.4f} (estimate {out['estimate_bpp']:.4f}), "
              f"PSNR {out['psnr']:.3f} dB, x_hat strictly inside (0, 1): {float(((x_cond > 0) & (x_cond < 1)).float().mean()):.2f}")


def gen_roi(scratch):
    from compressai.models.stem_roi import stem_roi, stem_roi_i
    ev = _import_script(scratch, "eval_stem_roi")
    imodel = closed_form_fill_scaled_(stem_roi_i(), "roi_i", ROI_CONV_SCALE).eval()
    pmodel = closed_form_fill_scaled_(stem_roi(), "roi_p", ROI_CONV_SCALE).eval()
    imodel.update(force=True), pmodel.update(force=True)
    qmap = closed_form_input("pixeleval:qmap", (1, 1, *SIZE), 0.0, 1.0)
    d = {"size": np.array(SIZE), "qmap": t2n(qmap)}
    print("roi chain")
    _chain(d, imodel, pmodel, lambda x: ev.inference_i(imodel, x, qmap), lambda x, c: ev.inference_p(pmodel, x, c, qmap))
    _tables(d, "roi_i", imodel), _tables(d, "roi_p", pmodel)
    save("pixel_eval_roi.npz", d)


def msh_fill_(m):
    return closed_form_fill_scaled_(m, "msh", 1.0)


def gen_baseline(scratch):
    from compressai.models.priors import MeanScaleHyperprior
    from compressai.models.stem_roi import stem_baseline
    ev = _import_script(scratch, "eval_stem_baseline")
    imodel = msh_fill_(MeanScaleHyperprior(64, 96)).eval()
    pmodel = closed_form_fill_scaled_(stem_baseline(), "base_p", ROI_CONV_SCALE).eval()
    imodel.update(force=True), pmodel.update(force=True)
    d = {"size": np.array(SIZE)}
    print("baseline chain")
    _chain(d, imodel, pmodel, lambda x: ev.inference_i(imodel, x), lambda x, c: ev.inference_p(pmodel, x, c))
    _tables(d, "msh", imodel), _tables(d, "base_p", pmodel)

    # one training-mode forward of MeanScaleHyperprior with injected noise, 64 x 64
    log = []
    tm = msh_fill_(MeanScaleHyperprior(64, 96)).train()
    tm.entropy_bottleneck._get_noise_cached = NoiseFeed("msh_eb", log)
    tm.gaussian_conditional._get_noise_cached = NoiseFeed("msh_gc", log)
    x = smooth_frames("pixeleval:msh", 1, 1, 64)[0]
    out = tm(x)
    d["train:x"] = t2n(x)
    d["train:x_hat"], d["train:y_hat"], d["train:y"] = t2n(out["x_hat"]), t2n(out["y_hat"]), t2n(out["y"])
    d["train:lik_y"], d["train:lik_z"] = t2n(out["likelihoods"]["y"]), t2n(out["likelihoods"]["z"])
    d["noise_log"] = np.array([f"{n}|{','.join(map(str, s))}" for n, s in log])
    d["keys:MeanScaleHyperprior"] = np.array([f"{k}|{','.join(map(str, v.shape))}" for k, v in MeanScaleHyperprior(64, 96).state_dict().items()])
    save("pixel_eval_baseline.npz", d)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    scratch, _ = import_reference()
    with torch.no_grad():
        gen_roi(scratch)
    gen_baseline(scratch)
