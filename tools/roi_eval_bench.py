#!/usr/bin/env python3
"""What the evaluation loop of the pixel-domain models costs on one synthetic 1080p frame (padded to 1088 x 1920), in two parts.

    python tools/roi_eval_bench.py [--passes 30] [--only coding,gop] [--out profiles/roi_eval_bench.json]

(a) coding: the device side and the copies of ONE one-shot coding call at the latent size of that frame (M = 192, 68 x 120), the host
    rANS coder left out (it is the same call on the same arrays either way).  Two routes in one process, alternating pass by pass:
      primitives  F.sub / F.round_ / .int() / F.build_indexes, then the two .cpu().contiguous() calls that transpose NHWC to NCHW
                  element by element on the host; for the decoder F.build_indexes + .cpu().contiguous(), one copy up, type_as + add
      kernels     F.symbols_pack (stem_symbols_pack) with its one copy down; F.symbols_pack without y, one copy up,
                  F.symbols_unpack (stem_symbols_unpack)
    Every pass is bracketed by HIP events and by a host clock that ends after the last result is on its side (the routes end in a
    copy, i.e. in a synchronisation); medians.  The two routes' outputs are compared bit for bit before anything is timed.
(b) gop: one GOP of 12 frames through evaluation.eval_gop_pixel with stem_roi_i + stem_roi (seeded default initialisation, uniform
    quality map 0.31) after a warm-up of one I and one P frame: seconds per I and per P frame, encode / decode split.

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

M, LH, LW = 192, 68, 120
FRAME = (1080, 1920)


def coding_inputs(F, dev):
    from spatiotemporalentropymodel_amd.models.spatiotemporalpriors import get_scale_table
    gen = torch.Generator(device=dev).manual_seed(3)
    table = torch.as_tensor(get_scale_table(), dtype=torch.float32).to(dev).contiguous()
    gp = torch.empty((1, LH, LW, 2 * M), device=dev)                                       # an entropy-parameter output: scales | means
    gp[..., :M] = torch.exp(torch.empty((1, LH, LW, M), device=dev).uniform_(-2.5, 3.0, generator=gen))
    gp[..., M:] = torch.randn((1, LH, LW, M), device=dev, generator=gen) * 2
    gp = gp.permute(0, 3, 1, 2)
    y = F.to_nhwc((torch.randn((1, M, LH, LW), device=dev, generator=gen) * 4).contiguous())
    return y, gp[:, :M], gp[:, M:], table


def routes(F, y, scales, means, table, bound=0.11):
    dev = y.device

    def prim_encode():
        m = F.dense_nhwc(means)
        sym = F.round_(F.sub(y, m)).int()
        idx = F.build_indexes(scales, table, bound)
        return sym.cpu().contiguous().numpy(), idx.int().cpu().contiguous().numpy()

    def kern_encode():
        sym, idx = F.symbols_pack(y, means, None, scales, table, bound).cpu().numpy()
        return sym, idx

    def prim_decode(sym_host):
        idx = F.build_indexes(scales, table, bound).int().cpu().contiguous().numpy()
        m = F.dense_nhwc(means)
        out = torch.from_numpy(sym_host).to(dev).type_as(m)
        out += m
        return idx, out

    def kern_decode(sym_host):
        idx = F.symbols_pack(None, scales=scales, table=table, scale_bound=bound)[1].cpu().numpy()
        return idx, F.symbols_unpack(torch.from_numpy(sym_host).to(dev), means)

    return {"encode": {"primitives": prim_encode, "kernels": kern_encode}, "decode": {"primitives": prim_decode, "kernels": kern_decode}}


def alternate(fns, passes, warmup=5):
    """per callable: medians of the HIP-event time and of the host time of a pass (milliseconds), alternating pass by pass"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(passes):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            ev[k].append(a.elapsed_time(b))
    return {k: {"event_ms_median": statistics.median(ev[k]), "wall_ms_median": statistics.median(wall[k]), "wall_ms_min": min(wall[k]),
                "wall_ms_p90": sorted(wall[k])[int(0.9 * (passes - 1))]} for k in fns}


def bench_coding(passes):
    import numpy as np
    from spatiotemporalentropymodel_amd import functional as F
    dev = torch.device("cuda", 0)
    y, scales, means, table = coding_inputs(F, dev)
    r = routes(F, y, scales, means, table)
    (sym_p, idx_p), (sym_k, idx_k) = r["encode"]["primitives"](), r["encode"]["kernels"]()
    same = bool(np.array_equal(sym_p, sym_k) and np.array_equal(idx_p, idx_k))
    sym_host = np.ascontiguousarray(sym_k)
    (di_p, out_p), (di_k, out_k) = r["decode"]["primitives"](sym_host), r["decode"]["kernels"](sym_host)
    same = same and bool(np.array_equal(di_p, di_k)) and bool(torch.equal(out_p.contiguous().view(torch.int32), out_k.contiguous().view(torch.int32)))
    if not same:
        sys.exit("tools/roi_eval_bench.py: the two routes disagree; nothing timed")
    enc = alternate(r["encode"], passes)
    dec = alternate({k: (lambda fn=fn: fn(sym_host)) for k, fn in r["decode"].items()}, passes)
    return {"shape": [1, M, LH, LW], "values": M * LH * LW, "passes": passes, "routes_agree_bit_for_bit": same, "encode": enc, "decode": dec,
            "note": "device work and copies of one coding call, host rANS coder excluded; event = HIP events around the pass, wall = host clock"}


def bench_gop(gop=12):
    from spatiotemporalentropymodel_amd import evaluation
    from spatiotemporalentropymodel_amd.models import stem_roi, stem_roi_i
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model_i, model_p = stem_roi_i().to(dev).eval(), stem_roi().to(dev).eval()
    model_i.update(force=True), model_p.update(force=True)
    base = torch.nn.functional.interpolate(smooth_frames("roi_eval_bench", 1, 1, 256)[0].to(dev), size=FRAME, mode="bilinear", align_corners=False)
    frames = [torch.roll(base[0], shifts=(t, 2 * t), dims=(1, 2)).clamp(0, 1).contiguous() for t in range(gop)]
    qmap = evaluation.quality_map("uniform", *FRAME, level=0.31, level_range=(0, 1))
    evaluation.eval_gop_pixel(model_i, model_p, frames[:2], qmaps=qmap, gop=gop, with_msssim=False)          # warm-up: every shape once
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = evaluation.eval_gop_pixel(model_i, model_p, frames, qmaps=qmap, gop=gop, with_msssim=False)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    out = {"frame": list(FRAME), "padded": [1088, 1920], "gop": gop, "seconds_total": total, "seconds_per_frame": total / gop,
           "bpp_ave": res["bpp_ave"], "psnr_ave": res["psnr_ave"], "weights": "seeded default initialisation (not a trained model)"}
    for kind in ("I", "P"):
        fr = [f for f in res["frames"] if f["type"] == kind]
        out[kind] = {"frames": len(fr), "encode_s_median": statistics.median(f["encoding_time"] for f in fr),
                     "decode_s_median": statistics.median(f["decoding_time"] for f in fr),
                     "y_bytes_mean": sum(len(f["strings"][0][0]) for f in fr) / len(fr)}
    out["note"] = "encode = compress + forward (the rate estimate), decode = decompress, as the scripts time them; metrics outside both"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=30)
    ap.add_argument("--only", default="coding,gop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/roi_eval_bench.py measures on an MI355X; no GPU found")
    parts = set(args.only.split(","))
    res = {"device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        if "coding" in parts:
            res["coding"] = bench_coding(args.passes)
            print(json.dumps({"coding": res["coding"]}))
        if "gop" in parts:
            res["gop"] = bench_gop()
            print(json.dumps({"gop": res["gop"]}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
