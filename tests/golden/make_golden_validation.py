#!/usr/bin/env python3
"""Generate tests/golden/validation.npz from the REFERENCE itself: stem/trainSTEM.py's own `validation` (:265-295), run as it is on
the CPU in float32 and in float64.  See make_golden.py for the import recipe.

    python tests/golden/make_golden_validation.py

The script is imported as a module.  It imports three names this image lacks and `validation` never touches: SummaryWriter (a
stand-in module is registered under torch.utils.tensorboard for the duration of the import) and, through stem/dataset_vidseq.py, the
torchvision / PIL names of its data loader (torchvision's stand-ins are import_reference's; an empty PIL.Image joins them).  Nothing of
the script but `validation` runs.

  models      make_golden.eval_gop_models: the small I-frame model (mbt2018) and SpatioTemporalPriorModel_Res(64, 96) on closed-form
              weights, as in eval_gop.npz
  test list   ITEMS items of NFRAMES frames [1,3,64,128] (the reference validates at batch 1, :148; the model needs frame sides that are
              multiples of 64: its hyper path halves the 16-fold reduced latents twice more): frames:<item> [NFRAMES,3,64,128]
  noise       mbt2018's getY adds noise in eval mode too (priors.py:691), once per getY call: draw k of the pass is
              closed_form_input("noise:iframe_gc:<k>") (make_golden.NoiseFeed), k = item * NFRAMES + frame.  Every call of `validation`
              starts again at k = 0, so the two calls below return the same loss.
  scheduler   ReduceLROnPlateau(dummy optimiser at lr 1e-4, "min", patience=0, factor=0.2), stepped by `validation` itself (:290), twice:
              the second loss is no improvement on the first, so the second call lowers the rate: lr [2] after each call
  loss64, loss32, steps64, steps32    the returned loss of each call [2] and criterion(...)["loss"] of every P step of the first call
              [ITEMS * (NFRAMES - 1)], float64 and float32 runs
  tie_margin  the smallest distance from a rounding tie (|frac(v) - 1/2|) of anything the float64 run passed to torch.round
  rel32       |loss32 - loss64| / loss64

  round_dist32  the largest |float32 - float64| of anything the two runs passed to torch.round: what tie_margin has to be read against

A candidate (seed of the frames) is kept if tie_margin >= TIE_MARGIN = 1e-3 and rel32 <= REL32_MAX = 1e-4 / 3: conditions the
reference alone has to meet -- a third of the project's 1e-4 parity gate, so that a float32 implementation as accurate as the
reference's own float32 run passes it with room -- checked here and recorded in the file.  A pass rounds about 38 000 values (six P
steps of 128 hyper-latents and twice 3072 latents, plus the I-frame model's), so the nearest of them lies about 0.5 / 38 000 =
1.3e-5 from a tie whatever the frames: where NO candidate of SEEDS clears TIE_MARGIN, the one with the largest tie_margin among those
that meet REL32_MAX is kept and the fixture says so (`margin_cleared` = 0), as make_golden_cheng.py does for its scale-table margin.
Only data is saved.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, NoiseFeed, eval_gop_models, import_reference, save, smooth_frames, t2n  # noqa: E402

ITEMS, NFRAMES, SIZE = 3, 3, (64, 128)
TIE_MARGIN, REL32_MAX = 1e-3, 1e-4 / 3
SEEDS = range(16)


def import_train_script(scratch, root_utils):
    os.makedirs(os.path.join(scratch, "PIL"), exist_ok=True)
    with open(os.path.join(scratch, "PIL", "__init__.py"), "w") as f:
        f.write("")
    with open(os.path.join(scratch, "PIL", "Image.py"), "w") as f:
        f.write("def open(*a, **k):\n    raise NotImplementedError\n")
    tv = os.path.join(scratch, "torchvision", "transforms", "__init__.py")
    with open(tv, "a") as f:                             # dataset_vidseq.py builds a Compose of ToTensor at import of its class bodies only
        f.write("class Compose:\n    def __init__(self, *a, **k):\n        pass\n")
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
    added = {"torch.utils.tensorboard": tb, "utils": root_utils}
    sys.modules.update(added)
    sys.path.insert(0, os.path.join(REF, "stem"))        # `from dataset_vidseq import get_loader`
    keep = os.environ.get("CUDA_VISIBLE_DEVICES")
    try:
        spec = importlib.util.spec_from_file_location("ref_trainSTEM", os.path.join(REF, "stem", "trainSTEM.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)                     # (sets CUDA_VISIBLE_DEVICES=0 at import: restored)
    finally:
        sys.path.remove(os.path.join(REF, "stem"))
        for k in added:
            sys.modules.pop(k, None)
        if keep is None:
            os.environ.pop("CUDA_VISIBLE_DEVICES", None)
        else:
            os.environ["CUDA_VISIBLE_DEVICES"] = keep
    return mod


def frames_of(seed):
    """ITEMS items of NFRAMES frames [1,3,64,128]: the top 64 rows of 128 x 128 smooth frames"""
    h, w = SIZE
    return [[f[:, :, :h, :w].contiguous() for f in smooth_frames(f"validation:{seed}:{i}", 1, NFRAMES, 128)] for i in range(ITEMS)]


def run(script, ref, items, dtype):
    from compressai.models.priors import JointAutoregressiveHierarchicalPriors
    from compressai.models.spatiotemporalpriors import SpatioTemporalPriorModel_Res
    imodel, stem = eval_gop_models(JointAutoregressiveHierarchicalPriors, SpatioTemporalPriorModel_Res)
    imodel, stem = imodel.to(dtype).train(), stem.to(dtype).train()                 # `validation` switches them itself
    loader = [[f.to(dtype) for f in item] for item in items]
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(dummy, "min", patience=0, factor=0.2)
    steps, margin, rounded = [], [float("inf")], []

    class Criterion(ref.EMLoss):                                                    # the reference's criterion, its per-step loss noted
        def forward(self, out, target):
            oc = super().forward(out, target)
            steps.append(float(oc["loss"]))
            return oc

    real_round = torch.round

    def watched_round(x, *a, **k):
        v = x.detach().double()
        margin[0] = min(margin[0], float(((v - torch.floor(v)) - 0.5).abs().min()))
        rounded.append(v.clone())
        return real_round(x, *a, **k)

    losses, lrs = [], []
    torch.round = watched_round
    try:
        for _ in range(2):
            imodel.gaussian_conditional._get_noise_cached = NoiseFeed("iframe_gc", [])          # every call starts at draw 0
            losses.append(float(script.validation(imodel, stem, loader, Criterion(), sched, "cpu")))
            lrs.append(dummy.param_groups[0]["lr"])
    finally:
        torch.round = real_round
    assert imodel.training and stem.training                                         # :292-293
    n = ITEMS * (NFRAMES - 1)
    assert len(steps) == 2 * n and steps[:n] == steps[n:] and losses[0] == losses[1]
    return np.array(losses), np.array(steps[:n]), np.array(lrs), margin[0], rounded


def main():
    scratch, ref = import_reference()
    script = import_train_script(scratch, ref)
    best = None
    for seed in SEEDS:
        items = frames_of(seed)
        loss64, steps64, lr64, margin, r64 = run(script, ref, items, torch.float64)
        loss32, steps32, lr32, _, r32 = run(script, ref, items, torch.float32)
        rel32 = abs(loss32[0] - loss64[0]) / abs(loss64[0])
        dist = max(float((a - b).abs().max()) for a, b in zip(r64, r32))
        assert len(r64) == len(r32)
        print(f"seed {seed}: loss64 {loss64[0]!r} loss32 {loss32[0]!r} rel32 {rel32:.3e} tie margin {margin:.3e} "
              f"(fp32 distance of the rounded values {dist:.3e}) lr {lr64}")
        if rel32 <= REL32_MAX and (best is None or margin > best[0]):
            best = (margin, seed, items, loss64, steps64, lr64, loss32, steps32, lr32, rel32, dist)
        if margin >= TIE_MARGIN and rel32 <= REL32_MAX:
            break
    if best is None:
        raise SystemExit("no candidate met REL32_MAX")
    margin, seed, items, loss64, steps64, lr64, loss32, steps32, lr32, rel32, dist = best
    cleared = margin >= TIE_MARGIN
    if not cleared:
        print(f"NO candidate clears a tie margin of {TIE_MARGIN}; keeping seed {seed} with {margin:.3e} ({margin / dist:.1f} x the fp32 distance)")
    assert lr64[0] == 1e-4 and lr64[1] == 1e-4 * 0.2 and (lr32 == lr64).all()
    assert abs(steps64.mean() - loss64[0]) <= 1e-12 * abs(loss64[0])
    d = {"seed": np.array([seed]), "cfg": np.array([ITEMS, NFRAMES, SIZE[0], SIZE[1]]), "loss64": loss64, "loss32": loss32, "steps64": steps64,
         "steps32": steps32, "lr": lr64, "tie_margin": np.array([margin]), "rel32": np.array([rel32]),
         "gates": np.array([TIE_MARGIN, REL32_MAX]),
         "margin_cleared": np.array([int(cleared)]), "round_dist32": np.array([dist])}
    for i, item in enumerate(items):
        d[f"frames:{i}"] = t2n(torch.cat(item))
    save("validation.npz", d)


if __name__ == "__main__":
    main()
