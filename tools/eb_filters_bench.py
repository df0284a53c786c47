"""Times of the EntropyBottleneck kernels for any `filters` tuple (csrc/eb_filters.hip) and, at (3, 3, 3, 3), of the specialised
kernels (csrc/entropy.hip) beside them.

    python tools/eb_filters_bench.py [--launches 50] [--out profiles/eb_filters.json]

Tuples (), (3, 3, 3), (3, 3, 3, 3), (2, 4, 8), (8,) * 6; shapes [16,192,4,4] and [16,192,16,16] (hyper-latents: launch latency
dominates) and [1,320,68,120] (the y of a FactorizedPrior at 1080p).  Per (tuple, shape): the forward in both modes, the backward
(dz and dpack) and the auxiliary loss with its gradient -- HIP events around every launch after a warm-up, median with the 10th and
90th percentile of `--launches` (>= 30).  At (3, 3, 3, 3) the general and the specialised kernel of each operation alternate in the
same loop, so that drift of the machine hits both alike, and both routes allocate their outputs inside the timed call.  Pack /
unpack launches are not part of the timed calls.  There is no gate on these numbers: the file is where the measured values live.

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

TUPLES = ((), (3, 3, 3), (3, 3, 3, 3), (2, 4, 8), (8,) * 6)
SHAPES = ((16, 192, 4, 4), (16, 192, 16, 16), (1, 320, 68, 120))
WARMUP = 5


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


def inputs(shape, filters, dev):
    """a bottleneck at init_scale 1 with every parameter perturbed (the recipe of tests/eb_filters_ref.py), latents of sigma 3"""
    from spatiotemporalentropymodel_amd import functional as F
    B, Cc, H, W = shape
    g = torch.Generator(device=dev).manual_seed(1)
    widths = (1, *filters, 1)
    cols = []
    for i in range(len(filters) + 1):
        init = float(torch.log(torch.expm1(torch.tensor(1.0 / widths[i + 1]))))
        cols.append(init + (torch.rand(Cc, widths[i + 1] * widths[i], device=dev, generator=g) - 0.5) * 0.6)
        cols.append(torch.rand(Cc, widths[i + 1], device=dev, generator=g) - 0.5)
        if i < len(filters):
            cols.append((torch.rand(Cc, widths[i + 1], device=dev, generator=g) - 0.5) * 0.8)
    pack = torch.cat(cols, dim=1).contiguous()
    assert pack.shape[1] == F.ebf_nparam(filters)
    z = F.empty_nhwc(B, Cc, H, W, dev).copy_(torch.randn(shape, device=dev, generator=g) * 3.0)
    noise = F.empty_nhwc(B, Cc, H, W, dev).copy_(torch.rand(shape, device=dev, generator=g) - 0.5)
    med = (torch.rand(Cc, device=dev, generator=g) - 0.5).contiguous()
    q = torch.stack([torch.full((Cc,), -8.0, device=dev), med, torch.full((Cc,), 8.0, device=dev)], dim=1).reshape(Cc, 1, 3).contiguous()
    target = torch.tensor([-20.7, 0.0, 20.7], device=dev)
    return pack, z, noise, med, q, target


def bench_case(shape, filters, launches):
    from spatiotemporalentropymodel_amd import functional as F
    dev = torch.device("cuda", 0)
    B, Cc, H, W = shape
    pack, z, noise, med, q, target = inputs(shape, filters, dev)
    z_hat, lik = F.ebf_forward(z, pack, filters, noise=noise)
    dlik = F.empty_nhwc(B, Cc, H, W, dev).copy_(-1.0 / (0.6931 * B * H * W) / lik)
    dq, loss = torch.empty_like(q), torch.empty(1, device=dev)
    special = filters == (3, 3, 3, 3)
    ops = {"forward_noise": {"general": lambda: F.ebf_forward(z, pack, filters, noise=noise)},
           "forward_eval": {"general": lambda: F.ebf_forward(z, pack, filters, medians=med)},
           "backward": {"general": lambda: F.ebf_backward(z_hat, pack, dlik, filters)},
           "aux_loss_grad": {"general": lambda: F.ebf_aux_loss_grad(q, pack, target, filters, dq, loss_out=loss)}}
    if special:
        ops["forward_noise"]["specialised"] = lambda: F.eb_forward(z, pack, noise=noise)
        ops["forward_eval"]["specialised"] = lambda: F.eb_forward(z, pack, medians=med)
        ops["backward"]["specialised"] = lambda: F.eb_backward(z_hat, pack, dlik)
        ops["aux_loss_grad"]["specialised"] = lambda: F.eb_aux_loss_grad(q, pack, target, dq, loss_out=loss)
    res = {"shape": list(shape), "filters": list(filters), "nparam": int(pack.shape[1]), "pixels_per_channel": B * H * W, "launches": launches}
    for name, routes in ops.items():
        res[name] = alternate(routes, launches)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eb_filters.json"))
    args = ap.parse_args()
    if args.launches < 30:
        sys.exit("eb_filters_bench: --launches must be at least 30")
    if not torch.cuda.is_available():
        sys.exit("eb_filters_bench: no GPU -- this tool measures on an MI355X and has no other mode")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "timing": "HIP events around every launch after a warm-up; median, 10th and 90th percentile; "
           "at (3, 3, 3, 3) the general and the specialised kernel alternate in one loop; every forward and backward, general or specialised, allocates its "
           "outputs inside the timed call; the auxiliary calls write into tensors handed in", "cases": []}
    for shape in SHAPES:
        for filters in TUPLES:
            res["cases"].append(bench_case(shape, filters, args.launches))
            c = res["cases"][-1]
            print(f"{shape} {filters}: " + "  ".join(f"{op} " + "/".join(f"{v['median_us']:.1f}" for v in c[op].values()) for op in
                                                      ("forward_noise", "forward_eval", "backward", "aux_loss_grad")) + " us", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
