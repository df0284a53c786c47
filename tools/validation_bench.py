#!/usr/bin/env python3
"""Times and launch counts of the validation pass (trainer.validate; stem/trainSTEM.py:265-295) on its two routes.

    python tools/validation_bench.py [--septuplets 16] [--rounds 7] [--out profiles/validation.json]

The bench's models (mbt2018 quality 4, SpatioTemporalPriorModel_Res(256, 192)) on synthetic 448 x 256 septuplets.  Five passes over
the same `--septuplets` sequences take turns in one loop after a warm-up round:

    generic_b1   module call + EMLoss at loader batch 1: the reference's configuration (:148) and the parent commit's arithmetic
    fused_b1     engine.eval_rate at loader batch 1
    fused_b16    engine.eval_rate with the sequences as batches of 16
    generic_b1_no_prefetch, fused_b1_no_prefetch    the batch-1 passes with prefetch=False (getY on the compute stream)

Per pass and round: wall time (host clock around the call, device idle before and after) and HIP-event time, both divided by the
number of septuplets; the file holds medians with the 10th-to-90th percentile band over `--rounds`, the ratios of the medians, and
the library launches of ONE P-frame eval forward with its loss on each route -- counted as tools/launch_list.py counts them (a
stand-in for the library that notes every entry point returning status 0), over all of include/*.h's entry points of
libstem_hip.so, torch operators not included.

No time is gated anywhere.  The rule for trainer.DEFAULT_VALIDATION_ROUTE is stated in the file: "fused" only if fused_b1's median
wall time is not above generic_b1's by more than generic_b1's own band.

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

H, W, NFRAMES = 256, 448, 7


class CountingLibrary:
    """stands in for the CDLL: every int-returning entry point that answers 0 (a launch or a copy was issued) is noted by name"""

    def __init__(self, lib, names):
        self._lib, self._names, self.calls = lib, names, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._names:
            return fn

        def counted(*args, _fn=fn, _name=name):
            rc = _fn(*args)
            if rc == 0:
                self.calls.append(_name)
            return rc
        return counted


def count_launches(fn):
    from spatiotemporalentropymodel_amd import _lib
    real = _lib.hip()
    names = set()
    for sig, restype in ((_lib._HIP_SIG, _lib._RESTYPE), (_lib._HIP_BATCH_SIG, {}), (_lib._HIP_BLOCKS_SIG, {}), (_lib._HIP_HYPERPRIOR_SIG, {}),
                         (_lib._HIP_EBF_SIG, {}), (_lib._HIP_GDN1_SIG, {}), (_lib._HIP_VALIDATION_SIG, {})):
        names |= {n for n in sig if n not in restype and not n.startswith(("stem_tape_", "stem_tuning", "stem_abi", "stem_last"))}
    proxy = CountingLibrary(real, names)
    _lib._hip = proxy
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib._hip = real
    return proxy.calls


def band(v):
    v = sorted(v)
    return {"median_ms": statistics.median(v), "p10_ms": v[int(0.1 * (len(v) - 1))], "p90_ms": v[int(round(0.9 * (len(v) - 1)))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--septuplets", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "validation.json"))
    args = ap.parse_args()
    from spatiotemporalentropymodel_amd import trainer as T
    from spatiotemporalentropymodel_amd.losses import EMLoss
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    from spatiotemporalentropymodel_amd.zoo import models
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    imodel = models["mbt2018"](quality=4).to(dev).eval()
    stem = SpatioTemporalPriorModel_Res().to(dev).train()
    n = args.septuplets
    g = torch.Generator(device=dev).manual_seed(1)
    seqs = [torch.rand(NFRAMES, 3, H, W, device=dev, generator=g) for _ in range(n)]
    loader_b1 = [[s[t:t + 1] for t in range(NFRAMES)] for s in seqs]
    loader_b16 = [[torch.stack([s[t] for s in seqs[i:i + 16]]) for t in range(NFRAMES)] for i in range(0, n, 16)]
    passes = {"generic_b1": lambda: T.validate(imodel, stem, loader_b1, route="generic"),
              "fused_b1": lambda: T.validate(imodel, stem, loader_b1, route="fused"),
              "fused_b16": lambda: T.validate(imodel, stem, loader_b16, route="fused"),
              # the same without the latent prefetcher (getY on the compute stream, in order): what the second stream is worth
              "generic_b1_no_prefetch": lambda: T.validate(imodel, stem, loader_b1, route="generic", prefetch=False),
              "fused_b1_no_prefetch": lambda: T.validate(imodel, stem, loader_b1, route="fused", prefetch=False)}
    results = {}
    for k, fn in passes.items():                         # warm-up: weights packed, workspaces and streams made
        results[k] = fn()
    wall, event = {k: [] for k in passes}, {k: [] for k in passes}
    for _ in range(args.rounds):
        for k, fn in passes.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3 / n)
            event[k].append(a.elapsed_time(b) / n)
    # launches of one P-frame eval forward with its loss
    with torch.no_grad():
        stem.eval()
        y_cond = imodel.getY(loader_b1[0][0])[1]
        y_cur = imodel.getY(loader_b1[0][1])[0]
        crit, acc = EMLoss(), torch.zeros(4, dtype=torch.float64, device=dev)
        eng = stem.engine()
        for fn in (lambda: crit(stem(y_cur, y_cond), loader_b1[0][1]), lambda: eng.eval_rate(y_cur, y_cond, H * W, acc=acc)):
            fn()                                         # packs are current
        generic_calls = count_launches(lambda: crit(stem(y_cur, y_cond), loader_b1[0][1]))
        fused_calls = count_launches(lambda: eng.eval_rate(y_cur, y_cond, H * W, acc=acc))
        stem.train()
    out = {"what": "trainer.validate per septuplet (7 frames of 448 x 256, 6 P-frame eval steps), mbt2018 q4 + SpatioTemporalPriorModel_Res(256,192)",
           "device": torch.cuda.get_device_name(0), "septuplets": n, "rounds": args.rounds,
           "wall_ms_per_septuplet": {k: band(v) for k, v in wall.items()},
           "hip_event_ms_per_septuplet": {k: band(v) for k, v in event.items()},
           "loss": {k: r["loss"] for k, r in results.items()},
           "launches_per_p_frame_eval_forward": {"generic": len(generic_calls), "fused": len(fused_calls)},
           "launch_names": {"generic": generic_calls, "fused": fused_calls}}
    gb, fb = out["wall_ms_per_septuplet"]["generic_b1"], out["wall_ms_per_septuplet"]["fused_b1"]
    out["ratio_fused_b1_over_generic_b1"] = {"wall": fb["median_ms"] / gb["median_ms"],
                                             "hip_event": out["hip_event_ms_per_septuplet"]["fused_b1"]["median_ms"] /
                                             out["hip_event_ms_per_septuplet"]["generic_b1"]["median_ms"]}
    out["ratio_fused_b1_over_generic_b1_no_prefetch"] = {"wall": out["wall_ms_per_septuplet"]["fused_b1_no_prefetch"]["median_ms"] /
                                                         out["wall_ms_per_septuplet"]["generic_b1_no_prefetch"]["median_ms"]}
    out["ratio_fused_b16_over_generic_b1"] = {"wall": out["wall_ms_per_septuplet"]["fused_b16"]["median_ms"] / gb["median_ms"]}
    not_slower = fb["median_ms"] <= gb["median_ms"] + (gb["p90_ms"] - gb["p10_ms"])
    out["default_route_rule"] = {"rule": "fused only if fused_b1's median wall time <= generic_b1's median + generic_b1's p10-p90 band",
                                 "fused_b1_not_slower": bool(not_slower), "route_none_means": "fused" if not_slower else "generic",
                                 "trainer.DEFAULT_VALIDATION_ROUTE": T.DEFAULT_VALIDATION_ROUTE}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "launch_names"}, indent=1))


if __name__ == "__main__":
    main()
