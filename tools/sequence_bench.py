"""What coding a sequence's GOPs side by side buys: evaluation.eval_sequence against evaluation.eval_gop, and the batched raster-order
encoder (stem_ar_encode_batch, csrc/ar.hip) against one stem_ar_encode_image call per image.

    python tools/sequence_bench.py [--frames 96] [--gop 12] [--concurrent 8] [--reps 10] [--only kernel,sequence] [--out profiles/sequence_bench.json]

1. kernel: G = 8 images of 68 x 120 latents, M = 192 (a 1080p frame; the models of `bench.py --config eval`, closed-form inputs): HIP
   events around one stem_ar_encode_batch call and around eight stem_ar_encode_image calls, alternating, `--reps` times each after a
   warm-up; medians, and whether the two gave the same symbols, indexes and reconstruction.
2. sequence: `--frames` synthetic 1080p frames (tools/metrics_bench.py's) at `--gop` through eval_gop and through
   eval_sequence(concurrent_gops=`--concurrent`), one pass each after a warm-up on the first frames, with_msssim=False: wall seconds
   per frame, the per-frame encoding / decoding times both report, split by frame type, and whether every string is the same.

Needs an MI355X: without a GPU it fails, it measures nothing on a CPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def _models(dev):
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    from spatiotemporalentropymodel_amd.zoo import models
    imodel = closed_form_fill_(models["mbt2018"](quality=4)).to(dev).eval()
    imodel.update(force=True)
    stem = closed_form_fill_(SpatioTemporalPriorModel_Res()).to(dev).eval()
    stem.update(force=True)
    return imodel, stem


def time_kernel(stem, reps, G=8, H=68, W=120):
    from spatiotemporalentropymodel_amd import codec, functional as F
    from spatiotemporalentropymodel_amd.weights import closed_form_input
    dev = torch.device("cuda", 0)
    M = stem.in_channels
    ar = codec._ARContext(stem, dev)

    def nhwc(tag, Cn, lo, hi):
        return codec._dense(F.to_nhwc(closed_form_input(tag, (G, Cn, H, W), lo, hi).to(dev)))

    target, hp, tp = nhwc("sb:y", M, -6.0, 6.0), nhwc("sb:hp", 2 * M, -1.0, 1.0), nhwc("sb:tp", 2 * M, -1.0, 1.0)
    start = torch.zeros((G, H + 4, W + 4, M), device=dev)
    start[:, 2:2 + H, 2:2 + W].permute(0, 3, 1, 2).copy_(target)
    bufs = {k: start.clone() for k in ("batch", "images")}
    out = {k: torch.empty((2, G, H * W, M), device=dev, dtype=torch.int32) for k in bufs}

    def batch():
        ar.encode_batch(bufs["batch"], G, H, W, *codec._prior_addrs(tp, hp, 0, H, W, M), out["batch"][0], out["batch"][1])

    def images():
        for g in range(G):
            ar.encode_wavefront(bufs["images"][g], H, W, *codec._prior_addrs(tp, hp, g, H, W, M), out["images"][0][g], out["images"][1][g])

    routes = {"batch": batch, "images": images}
    for fn in routes.values():                       # warm-up; this first pass is also the comparison
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out["batch"], out["images"]) and torch.equal(bufs["batch"], bufs["images"]))
    events = []
    for _ in range(reps):
        for k, fn in routes.items():                 # alternating
            bufs[k].copy_(start)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events.append((k, a, b))
        torch.cuda.synchronize()                     # the queue of one pass (3200 or 12800 launches) drains before the next is timed
    ms = {k: sorted(a.elapsed_time(b) for kk, a, b in events if kk == k) for k in routes}
    med = {k: statistics.median(v) for k, v in ms.items()}
    steps = W + 3 * (H - 1)
    return {"shape": {"G": G, "H": H, "W": W, "M": M}, "reps": reps, "wavefront_steps": steps, "launches": {"batch": 5 * steps, "images": 5 * steps * G},
            "median_ms": {"stem_ar_encode_batch, one call": med["batch"], f"stem_ar_encode_image x {G}": med["images"]},
            "min_ms": {k: v[0] for k, v in ms.items()}, "max_ms": {k: v[-1] for k, v in ms.items()},
            "median_ms_per_image": {k: v / G for k, v in med.items()}, "images_over_batch": med["images"] / med["batch"],
            "us_per_step": {k: 1e3 * v / steps for k, v in med.items()}, "same_symbols_indexes_reconstruction": same}


def time_sequence(imodel, stem, n_frames, gop, concurrent):
    from spatiotemporalentropymodel_amd import evaluation
    dev = torch.device("cuda", 0)
    Hh, Ww = 1080, 1920
    yy, xx = torch.meshgrid(torch.arange(Hh, device=dev), torch.arange(Ww, device=dev), indexing="ij")
    frames = [torch.stack([0.5 + 0.4 * torch.sin((xx + 3 * t) / (40.0 + 10 * c)) * torch.cos((yy + t) / (55.0 - 5 * c)) for c in range(3)]) for t in range(n_frames)]
    warm = frames[:2] + frames[gop:gop + 2]
    evaluation.eval_gop(imodel, stem, warm[:2], gop=gop, with_msssim=False)              # every kernel and both decoder forms once
    evaluation.eval_sequence(imodel, stem, warm, gop=2, concurrent_gops=2, with_msssim=False)
    runs = {"eval_gop": lambda: evaluation.eval_gop(imodel, stem, frames, gop=gop, with_msssim=False),
            f"eval_sequence(concurrent_gops={concurrent})": lambda: evaluation.eval_sequence(imodel, stem, frames, gop=gop, concurrent_gops=concurrent,
                                                                                               with_msssim=False)}
    res, strings = {}, {}
    for name, fn in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        per_type = {}
        for kind in ("I", "P"):
            fs = [f for f in r["frames"] if f["type"] == kind]
            if fs:
                per_type[kind] = {"frames": len(fs), "encoding_s_per_frame": sum(f["encoding_time"] for f in fs) / len(fs),
                                  "decoding_s_per_frame": sum(f["decoding_time"] for f in fs) / len(fs)}
        coded = sum(f["encoding_time"] + f["decoding_time"] for f in r["frames"])
        res[name] = {"wall_s": wall, "wall_s_per_frame": wall / n_frames, "coding_s_per_frame": coded / n_frames,
                     "outside_the_timed_regions_s_per_frame": (wall - coded) / n_frames, "by_type": per_type, "bpp_ave": r["bpp_ave"], "psnr_ave": r["psnr_ave"]}
        strings[name] = [f["strings"] for f in r["frames"]]
        del r
    a, b = list(res)
    return {"workload": f"{n_frames} synthetic {Ww}x{Hh} frames, gop {gop}, models of bench.py --config eval, with_msssim=False, one pass each in one process",
            "runs": res, "eval_gop_over_eval_sequence_wall": res[a]["wall_s"] / res[b]["wall_s"],
            "eval_gop_over_eval_sequence_coding": res[a]["coding_s_per_frame"] / res[b]["coding_s_per_frame"], "same_strings": strings[a] == strings[b]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--gop", type=int, default=12)
    ap.add_argument("--concurrent", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="kernel,sequence", help="comma-separated parts to run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sequence_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sequence_bench: no GPU -- this tool measures on an MI355X and has no other mode")
    only = set(args.only.split(","))
    if not only or only - {"kernel", "sequence"}:
        sys.exit("sequence_bench: --only takes kernel, sequence")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        imodel, stem = _models(dev)
        if "kernel" in only:
            res["kernel"] = time_kernel(stem, args.reps)
        if "sequence" in only:
            res["sequence"] = time_sequence(imodel, stem, args.frames, args.gop, args.concurrent)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
