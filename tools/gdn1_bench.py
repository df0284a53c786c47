"""Times of the GDN1 kernels (csrc/gdn1.hip: stem_gdn1_fwd / stem_gdn1_bwd) with the GDN kernels (stem_gdn_fwd / stem_gdn_bwd) beside
them as the yardstick: the same shapes, the same process, the same loop.

    python tools/gdn1_bench.py [--launches 40] [--out profiles/gdn1.json]

Shapes [1,192,540,960] (g_a.0's output at 1080p) and [16,128,128,128] (the ROI ladder), forward and inverse.  Per shape the four
routes -- gdn1 forward, gdn forward, gdn1 backward, gdn backward (dx, dbeta and dgamma, workspaces allocated once outside the timed
calls) -- take turns in one loop after a warm-up, HIP events around every call; the file holds the median with the 10th and 90th
percentile of `--launches` per route, and the ratio of the medians.  There is no gate on these numbers: the file is where the
measured values live.

Needs an MI355X: without a GPU it fails, it measures nothing on a CPU.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

SHAPES = ((1, 192, 540, 960), (16, 128, 128, 128))
WARMUP = 3


def alternate(routes, launches):
    """{name: fn} -> {name: {median_us, p10_us, p90_us}}: the routes take turns, one pair of events around every call"""
    for _ in range(WARMUP):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    events = []
    for _ in range(launches):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events.append((k, a, b))
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for k, a, b in events:
        times[k].append(a.elapsed_time(b) * 1e3)
    out = {}
    for k, v in times.items():
        v.sort()
        out[k] = {"median_us": statistics.median(v), "p10_us": v[int(0.1 * (len(v) - 1))], "p90_us": v[int(0.9 * (len(v) - 1))]}
    return out


def routes(shape, inverse, dev):
    from spatiotemporalentropymodel_amd import _lib
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd.layers import GDN
    B, Cc, H, W = shape
    lib, npix = _lib.hip(), B * H * W
    g = torch.Generator(device=dev).manual_seed(3)
    x = F.empty_nhwc(B, Cc, H, W, dev).copy_(torch.randn((B, Cc, H, W), device=dev, generator=g))
    dy = F.empty_nhwc(B, Cc, H, W, dev).copy_(torch.randn((B, Cc, H, W), device=dev, generator=g))
    m = GDN(Cc, inverse=inverse).to(dev)
    beta = m.beta.detach().contiguous()
    gamma = (m.gamma.detach() + 0.02 * torch.rand((Cc, Cc), device=dev, generator=g)).contiguous()      # dense, as after training
    y, dx = F.empty_nhwc(B, Cc, H, W, dev), F.empty_nhwc(B, Cc, H, W, dev)
    dbeta, dgamma = torch.empty_like(beta), torch.empty_like(gamma)
    n1, n0 = int(lib.stem_gdn1_bwd_workspace_bytes(npix, Cc)), int(lib.stem_gdn_bwd_workspace_bytes(B, H, W, Cc))
    ws1 = torch.empty((n1 + 3) // 4, device=dev, dtype=torch.float32)
    ws0 = torch.empty((n0 + 3) // 4, device=dev, dtype=torch.float32)
    p = lambda t: t.data_ptr()          # noqa: E731
    inv, bm = int(inverse), 1e-6

    def chk(rc):
        if rc:
            raise RuntimeError(lib.stem_last_error().decode())
    return {
        "gdn1_fwd": lambda: chk(lib.stem_gdn1_fwd(p(x), Cc, p(beta), p(gamma), p(y), Cc, npix, Cc, inv, bm, F._stream())),
        "gdn_fwd": lambda: chk(lib.stem_gdn_fwd(p(x), Cc, p(beta), p(gamma), p(y), Cc, B, H, W, Cc, inv, bm, F._stream())),
        "gdn1_bwd": lambda: chk(lib.stem_gdn1_bwd(p(x), Cc, p(dy), Cc, p(beta), p(gamma), p(dx), Cc, p(dbeta), p(dgamma), npix, Cc, inv, bm,
                                                  p(ws1), n1, F._stream())),
        "gdn_bwd": lambda: chk(lib.stem_gdn_bwd(p(x), Cc, p(dy), Cc, p(beta), p(gamma), p(dx), Cc, p(dbeta), p(dgamma), B, H, W, Cc, inv, bm,
                                                p(ws0), n0, F._stream())),
    }, {"gdn1_bwd_workspace_bytes": n1, "gdn_bwd_workspace_bytes": n0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gdn1.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/gdn1_bench.py measures on an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": WARMUP, "cases": []}
    for shape in SHAPES:
        for inverse in (False, True):
            fns, ws = routes(shape, inverse, dev)
            t = alternate(fns, args.launches)
            case = {"shape": list(shape), "inverse": inverse, **ws, "times": t,
                    "fwd_gdn1_over_gdn": t["gdn1_fwd"]["median_us"] / t["gdn_fwd"]["median_us"],
                    "bwd_gdn1_over_gdn": t["gdn1_bwd"]["median_us"] / t["gdn_bwd"]["median_us"]}
            res["cases"].append(case)
            print(f"{shape} inverse={inverse}: " + "  ".join(f"{k} {v['median_us']:.0f} us [{v['p10_us']:.0f}, {v['p90_us']:.0f}]" for k, v in t.items()) +
                  f"  fwd x{case['fwd_gdn1_over_gdn']:.2f}  bwd x{case['bwd_gdn1_over_gdn']:.2f}", flush=True)
            del fns
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
