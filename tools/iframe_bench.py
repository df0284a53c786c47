#!/usr/bin/env python3
"""I-frame models at 1088 x 1920: getY, getX, compress and decompress of mbt2018, cheng2020-anchor and cheng2020-attn (quality 4),
and the block kernels of csrc/resblock.hip alone at the shapes g_s gives them; analysis, synthesis, compress and decompress of
bmshj2018-factorized and bmshj2018-hyperprior (which have no getY / getX); the two routes of GaussianConditional.forward(means=None).

    python tools/iframe_bench.py                                     print the figures
    python tools/iframe_bench.py --json profiles/cheng_iframe_1080p.json
    python tools/iframe_bench.py --models bmshj2018-factorized bmshj2018-hyperprior --no-kernels --json profiles/bmshj_iframe_1080p.json
    python tools/iframe_bench.py --gc-route profiles/gc_scale_route.json      only the zero-mean route against the zero-tensor route

HIP events on the launching stream, warm-up first, the median of the timed passes.  Each kernel's achieved bytes/s (what it must
read plus what it must write, over its time) stands beside stem_copy_channels moving the same number of bytes: the yardstick of a
pass that only streams.  Closed-form weights, tamed as in tests/golden/make_golden_cheng.py so that activations stay finite;
nothing here is a gate.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from spatiotemporalentropymodel_amd import functional as F  # noqa: E402
from spatiotemporalentropymodel_amd import layers as L  # noqa: E402
from spatiotemporalentropymodel_amd import zoo  # noqa: E402
from spatiotemporalentropymodel_amd.weights import closed_form_fill_, smooth_frames  # noqa: E402

H, W, N = 1088, 1920, 192
DEV = "cuda:0"


def timed(fn, warmup, passes):
    """median milliseconds of `passes` calls, HIP events around each"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def build(name):
    m = closed_form_fill_(zoo.models[name](quality=4))
    with torch.no_grad():
        if name == "mbt2018":                                   # tests/golden/make_golden.py:gen_iframe_codec
            m.g_a[6].weight.mul_(4.0), m.g_a[6].bias.mul_(4.0), m.g_s[0].weight.mul_(0.25)
        elif name.startswith("bmshj2018"):                      # tests/golden/make_golden_bmshj.py:build
            m.g_s[0].weight.mul_(0.25)
        else:                                                   # tests/golden/make_golden_cheng.py:build
            (last,) = [c for c in m.g_a.children() if isinstance(c, L.Conv2d)]
            last.weight.mul_(0.03), last.bias.mul_(0.03)
            for p in m.g_s.parameters():
                if p.dim() == 4:
                    p.mul_(0.5)
    m = m.to(DEV).eval()
    m.update(force=True)
    return m


def bench_models(args):
    x = smooth_frames("iframe_bench", 1, 1, W)[0][:, :, :H, :].contiguous().to(DEV)
    res = {}
    for name in args.models:
        m = build(name)
        with torch.no_grad():
            y = m.g_a(x)
            y_hat = F.round_(F.dense_nhwc(y))
            if hasattr(m, "getY"):
                r = {"getY_ms": timed(lambda: m.getY(x), args.warmup, args.passes), "getX_ms": timed(lambda: m.getX(y_hat), args.warmup, args.passes)}
            else:                                                # the bmshj2018 models: the transforms themselves, and the eval forward
                r = {"g_a_ms": timed(lambda: m.g_a(x), args.warmup, args.passes),
                     "g_s_ms": timed(lambda: F.to_nchw(m.g_s(y_hat), clamp01=True), args.warmup, args.passes),
                     "forward_ms": timed(lambda: m(x), args.warmup, args.passes)}
            enc = m.compress(x)                                  # warm-up: first use of the coding kernels, the decoder's self-check
            m.decompress(enc["strings"], enc["shape"])
            r["compress_ms"] = timed(lambda: m.compress(x), 0, args.codec_passes)
            r["decompress_ms"] = timed(lambda: m.decompress(enc["strings"], enc["shape"]), 0, args.codec_passes)
            r["bytes"] = sum(len(s[0]) for s in enc["strings"])
        res[name] = r
        print("%-21s " % name + "  ".join("%s %.2f" % (k[:-3] + " ms", v) if k.endswith("_ms") else "(%d bytes)" % v for k, v in r.items()))
        del m
        torch.cuda.empty_cache()
    return res


def _copy_gbs(nbytes, args):
    """stem_copy_channels reading + writing `nbytes` in all: dense [npix, 192] tensors"""
    npix = max(1, nbytes // 8 // N)
    src, dst = F.empty_nhwc(1, N, 1, npix, DEV).normal_(), F.empty_nhwc(1, N, 1, npix, DEV)
    ms = timed(lambda: F.copy_channels(src, dst), args.warmup, args.passes)
    return npix * N * 8 / ms / 1e6


def bench_kernels(args):
    rows = []

    def row(name, shape, nbytes, fn):
        ms = timed(fn, args.warmup, args.passes)
        gbs, copy = nbytes / ms / 1e6, _copy_gbs(nbytes, args)
        rows.append({"kernel": name, "shape": shape, "bytes": nbytes, "ms": ms, "GB_per_s": gbs, "copy_channels_GB_per_s": copy, "of_copy": gbs / copy})
        print("%-34s %-22s %8.3f ms  %7.1f GB/s  (copy_channels on the same bytes: %7.1f GB/s, %.2f of it)" % (name, shape, ms, gbs, copy, gbs / copy))

    with torch.no_grad():
        # the three ResidualBlockUpsample stages of g_s (N = 192, r = 2) and its last layer (12 -> 3 channels)
        for h, w, c in ((H // 16, W // 16, N), (H // 8, W // 8, N), (H // 4, W // 4, N), (H // 2, W // 2, 3)):
            x = F.empty_nhwc(1, c * 4, h, w, DEV).normal_()
            add, g = F.empty_nhwc(1, c, 2 * h, 2 * w, DEV).normal_(), F.empty_nhwc(1, c, 2 * h, 2 * w, DEV).normal_()
            n = x.numel() * 4
            shape = f"[{h}x{w}x{c * 4}] r=2"
            if c == 3:
                row("pixel_shuffle", shape, 2 * n, lambda: F.pixel_shuffle(x, 2))
                row("pixel_shuffle_backward", shape, 2 * n, lambda: F.pixel_shuffle_backward(g, 2))
                continue
            row("pixel_shuffle + lrelu", shape, 2 * n, lambda: F.pixel_shuffle(x, 2, 0.01))
            row("pixel_shuffle + addend", shape, 3 * n, lambda: F.pixel_shuffle(x, 2, 1.0, add))
            row("pixel_shuffle_backward + lrelu", shape, 3 * n, lambda: F.pixel_shuffle_backward(g, 2, x, 0.01))
        # the attention blocks of g_s: at the latent resolution and at 1/4
        for h, w in ((H // 16, W // 16), (H // 4, W // 4)):
            a, b, x, g = (F.empty_nhwc(1, N, h, w, DEV).normal_() for _ in range(4))
            n = a.numel() * 4
            shape = f"[{h}x{w}x{N}]"
            row("add_act", shape, 3 * n, lambda: F.add_act(a, b))
            row("add_act_backward", shape, 3 * n, lambda: F.add_act_backward(a, g))
            row("gate", shape, 4 * n, lambda: F.gate(a, b, x))
            row("gate_backward", shape, 5 * n, lambda: F.gate_backward(a, b, g))
    return rows


GC_ROUTE_SHAPES = ((1, 320, 68, 120), (16, 192, 16, 16))          # the latents of one 1088 x 1920 frame (M = 320); a training batch


def bench_gc_route(args):
    """GaussianConditional.forward(y, scales) in training mode and its backward, both ways, in one process, alternating: the
    zero-tensor route (memset of a mean tensor, noise pass, stem_gc_forward; stem_gc_backward with a dmeans nobody reads, stem_add)
    against the zero-mean route (stem_gc_scale_forward; stem_gc_scale_backward), allocations included as the modules make them.
    Per shape and direction: the median over the rounds of each route's median over `passes` calls."""
    rows = []
    for shape in GC_ROUTE_SHAPES:
        B, C, Hh, Ww = shape
        y, dlik, dout = (F.empty_nhwc(B, C, Hh, Ww, DEV).normal_() for _ in range(3))
        sc = F.empty_nhwc(B, C, Hh, Ww, DEV).uniform_(0.05, 4.0)

        def old_fwd():
            mu = torch.zeros_like(y, memory_format=torch.preserve_format)
            return F.gc_forward(y, sc, mu, noise=F.uniform_noise_like(y, 0x5713, 0)), mu

        def new_fwd():
            return F.gc_scale_forward(y, sc, "noise", seed=0x5713, offset=0)

        (out, _), mu = old_fwd()

        def old_bwd():
            dgp, dy = F.empty_nhwc(B, 2 * C, Hh, Ww, DEV), F.empty_nhwc(B, C, Hh, Ww, DEV)
            F.gc_backward(out, sc, mu, dlik, dgp[:, :C], dgp[:, C:], dy=dy)
            return F.add(dy, dout)

        def new_bwd():
            dsc, dy = F.empty_nhwc(B, C, Hh, Ww, DEV), F.empty_nhwc(B, C, Hh, Ww, DEV)
            F.gc_scale_backward(out, sc, dlik, dscales=dsc, dy=dy, dout=dout)
            return dy

        assert bool((new_fwd()[0] == old_fwd()[0][0]).all()) and torch.equal(new_bwd(), old_bwd())
        for direction, old, new in (("forward", old_fwd, new_fwd), ("backward", old_bwd, new_bwd)):
            per_round = {"zero_tensor_route": [], "zero_mean_route": []}
            for _ in range(args.rounds):
                per_round["zero_tensor_route"].append(timed(old, args.warmup, args.passes))
                per_round["zero_mean_route"].append(timed(new, args.warmup, args.passes))
            row = {"shape": list(shape), "direction": direction, "launches": {"zero_tensor_route": 3 if direction == "forward" else 2, "zero_mean_route": 1}}
            for k, v in per_round.items():
                row[k + "_ms"] = statistics.median(v)
                row[k + "_rounds_ms"] = v
            rows.append(row)
            print("gc route %-18s %-8s zero tensor %.4f ms  zero mean %.4f ms  (rounds: %s | %s)" %
                  (list(shape), direction, row["zero_tensor_route_ms"], row["zero_mean_route_ms"],
                   " ".join("%.4f" % v for v in per_round["zero_tensor_route"]), " ".join("%.4f" % v for v in per_round["zero_mean_route"])))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--models", nargs="*", default=["mbt2018", "cheng2020-anchor", "cheng2020-attn", "bmshj2018-factorized", "bmshj2018-hyperprior"],
                    choices=["mbt2018", "cheng2020-anchor", "cheng2020-attn", "bmshj2018-factorized", "bmshj2018-hyperprior"], help="the zoo entries to time")
    ap.add_argument("--no-kernels", action="store_true", help="skip the block kernels of csrc/resblock.hip")
    ap.add_argument("--gc-route", default=None, metavar="JSON", help="time the two routes of GaussianConditional.forward(means=None), write them here, and stop")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two routes (--gc-route)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=11, help="timed passes of getY / getX and of each kernel")
    ap.add_argument("--codec-passes", type=int, default=3, help="timed passes of compress / decompress (seconds each)")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--json", default=None, help="write the figures to this file")
    args = ap.parse_args()
    res = {"size": [H, W], "quality": 4, "warmup": args.warmup, "passes": args.passes, "codec_passes": args.codec_passes,
           "device": torch.cuda.get_device_name(0)}
    if args.gc_route:
        out = {"warmup": args.warmup, "passes": args.passes, "rounds": args.rounds, "device": res["device"], "timing": "HIP events around each call, "
               "median of the passes per round, routes alternating round by round", "rows": bench_gc_route(args)}
        os.makedirs(os.path.dirname(os.path.abspath(args.gc_route)), exist_ok=True)
        with open(args.gc_route, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    if not args.no_kernels:
        res["kernels"] = bench_kernels(args)
    if not args.kernels_only:
        res["models"] = bench_models(args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
