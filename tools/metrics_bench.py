"""Time of the MS-SSIM / MSE kernel (stem_ms_ssim, csrc/msssim.hip) and what each `with_msssim` route adds to the evaluation loop.

    python tools/metrics_bench.py [--launches 60] [--passes 3] [--only kernel,grad,eval_gop] [--out profiles/metrics_bench.json]

1. stem_ms_ssim at [1,3,1080,1920] and [8,3,1080,1920]: HIP events around every launch after a warm-up, the median of `--launches`
   (>= 50).  Bytes moved are computed from the shapes -- both images read once, the pooled planes of scales 2-5 written and read
   once -- and reported over that time as a share of the achievable HBM rate (halo re-reads are served by the caches and are not
   counted: the figure is the algorithm's traffic over the kernel's time, not a counter).
2. evaluation.eval_gop on one synthetic 1080p GOP of 12 (the models of `bench.py --config eval`) with with_msssim = False, True and
   "device", alternating, `--passes` passes each: wall time per GOP and the cost each metric route adds per frame over False.
3. forward + backward of the differentiable metric (stem_ms_ssim + stem_ms_ssim_bwd, as losses.ms_ssim runs them for a gradient
   with respect to x_hat) at [16,3,256,256] and [1,3,1080,1920], and beside it torch autograd through the fp32 body of
   evaluation.ms_ssim on the same GPU (what a user had before): HIP events around every forward + backward after a warm-up, the
   two routes alternating, medians; the largest difference of the two gradients over the largest gradient is reported with them.

Needs an MI355X: without a GPU it fails, it measures nothing on a CPU.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

HBM_ACHIEVABLE = 6.3e12        # bytes/s a streaming kernel reaches on an MI355X (8 TB/s peak)


def traffic_bytes(B, Cc, H, W):
    planes, total, h, w = B * Cc, 0, H, W
    for s in range(5):
        total += 2 * planes * h * w * 4 * (1 if s == 0 else 2)      # x and y: read (scale 1); written, then read (scales 2-5)
        h, w = (h + 1) // 2, (w + 1) // 2
    return total


def time_kernel(shape, launches, warmup=10):
    from spatiotemporalentropymodel_amd import _lib, functional as F
    dev = torch.device("cuda", 0)
    B, Cc, H, W = shape
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(shape, device=dev, generator=g)
    y = (x + 0.02 * torch.randn(shape, device=dev, generator=g)).clamp(0, 1)
    n = C.c_size_t(0)
    _lib.check(_lib.hip().stem_ms_ssim_workspace(B, Cc, H, W, C.byref(n)))
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
    out, mse, terms = (torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, Cc, 5, device=dev))

    def launch():
        _lib.check(_lib.hip().stem_ms_ssim(x.data_ptr(), y.data_ptr(), B, Cc, H, W, 1.0, ws.data_ptr(), ws.numel(), out.data_ptr(), mse.data_ptr(),
                                           terms.data_ptr(), F._stream()))
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in events:
        a.record()
        launch()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in events)
    med = statistics.median(ms) * 1e-3
    nbytes = traffic_bytes(*shape)
    return {"shape": list(shape), "launches": launches, "kernels_per_call": 6, "median_us": med * 1e6, "min_us": ms[0] * 1e3, "p90_us": ms[int(0.9 * (launches - 1))] * 1e3,
            "bytes_from_shapes": nbytes, "workspace_bytes": n.value, "bytes_per_s": nbytes / med, "share_of_achievable_hbm_6.3TBps": nbytes / med / HBM_ACHIEVABLE,
            "ms_ssim": out.tolist(), "mse": mse.tolist()}


def torch_ms_ssim(x, y, data_range=1.0):
    """the fp32 body of evaluation.ms_ssim on the tensors' own device, graph attached -> [B]"""
    from spatiotemporalentropymodel_amd.evaluation import _MS_WEIGHTS, _gauss_filter, _gauss_window
    win = _gauss_window().to(x.device)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    terms = []
    for level in range(5):
        mu1, mu2 = _gauss_filter(x, win), _gauss_filter(y, win)
        s11 = _gauss_filter(x * x, win) - mu1 * mu1
        s22 = _gauss_filter(y * y, win) - mu2 * mu2
        s12 = _gauss_filter(x * y, win) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
        if level < 4:
            terms.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = [s % 2 for s in x.shape[2:]]
            x = torch.nn.functional.avg_pool2d(x, kernel_size=2, padding=pad)
            y = torch.nn.functional.avg_pool2d(y, kernel_size=2, padding=pad)
        else:
            ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
            terms.append(torch.relu(ssim_map.flatten(2).mean(-1)))
    w = torch.tensor(_MS_WEIGHTS, device=x.device).view(-1, 1, 1)
    return torch.prod(torch.stack(terms) ** w, dim=0).mean(1)


def time_grad(shape, launches, warmup=5):
    from spatiotemporalentropymodel_amd import functional as F
    dev = torch.device("cuda", 0)
    B = shape[0]
    g = torch.Generator(device=dev).manual_seed(1)
    target = torch.rand(shape, device=dev, generator=g)
    x_hat = (target + 0.02 * torch.randn(shape, device=dev, generator=g)).clamp(0, 1)
    up = torch.full((B,), -1.0 / B, device=dev)
    got = {}

    def hip():
        _, ws = F.ms_ssim_forward_keep(x_hat, target)
        got["hip"] = F.ms_ssim_backward(x_hat, target, up, fwd_workspace=ws)

    def autograd():
        xr = x_hat.clone().requires_grad_(True)
        torch_ms_ssim(xr, target).backward(up)
        got["torch"] = xr.grad

    routes = {"hip": hip, "torch": autograd}
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    events = []
    for _ in range(launches):
        for k, fn in routes.items():                                                   # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events.append((k, a, b))
    torch.cuda.synchronize()
    for k, a, b in events:
        times[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in times.items()}
    diff = float((got["hip"] - got["torch"]).abs().max() / got["torch"].abs().max())
    return {"shape": list(shape), "launches": launches, "hip_kernels_per_call": 12,
            "median_ms": {"stem_ms_ssim + stem_ms_ssim_bwd": med["hip"], "torch autograd, fp32 body of evaluation.ms_ssim": med["torch"]},
            "min_ms": {k: min(v) for k, v in times.items()}, "p90_ms": {k: sorted(v)[int(0.9 * (launches - 1))] for k, v in times.items()},
            "torch_over_hip": med["torch"] / med["hip"], "max_gradient_difference_over_max_gradient": diff}


def time_eval(passes):
    from spatiotemporalentropymodel_amd import evaluation
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    from spatiotemporalentropymodel_amd.zoo import models
    dev = torch.device("cuda", 0)
    Hh, Ww, GOP = 1080, 1920, 12
    imodel = closed_form_fill_(models["mbt2018"](quality=4)).to(dev).eval()
    imodel.update(force=True)
    stem = closed_form_fill_(SpatioTemporalPriorModel_Res()).to(dev).eval()
    stem.update(force=True)
    yy, xx = torch.meshgrid(torch.arange(Hh, device=dev), torch.arange(Ww, device=dev), indexing="ij")
    frames = [torch.stack([0.5 + 0.4 * torch.sin((xx + 3 * t) / (40.0 + 10 * c)) * torch.cos((yy + t) / (55.0 - 5 * c)) for c in range(3)]) for t in range(GOP)]
    modes = [False, True, "device"]
    evaluation.eval_gop(imodel, stem, frames, gop=GOP, with_msssim="device")          # warm-up: every kernel and both metric routes once
    evaluation.eval_gop(imodel, stem, frames[:2], gop=GOP, with_msssim=True)
    wall = {repr(m): [] for m in modes}
    last = {}
    for _ in range(passes):
        for m in modes:                                                                # alternating: drift of the box hits all three alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evaluation.eval_gop(imodel, stem, frames, gop=GOP, with_msssim=m)
            torch.cuda.synchronize()
            wall[repr(m)].append(time.perf_counter() - t0)
            last[repr(m)] = res
    med = {k: statistics.median(v) for k, v in wall.items()}
    add_host = (med["True"] - med["False"]) / GOP
    add_dev = (med["'device'"] - med["False"]) / GOP
    spread = max(wall["False"]) - min(wall["False"])
    return {"workload": f"evaluation.eval_gop, one {Ww}x{Hh} GOP of {GOP}, models of bench.py --config eval", "passes": passes, "wall_s_per_gop": wall, "median_s_per_gop": med,
            "spread_of_False_s_per_gop": spread,
            "added_s_per_frame": {"True (host evaluation.ms_ssim)": add_host, "'device' (stem_ms_ssim + one read of two scalars)": add_dev},
            "device_over_host_added_cost": add_dev / add_host if add_host > 0 else None,
            "msssim_ave": {k: v["msssim_ave"] for k, v in last.items()}, "psnr_ave": {k: v["psnr_ave"] for k, v in last.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--only", default="kernel,grad,eval_gop", help="comma-separated parts to run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "metrics_bench.json"))
    args = ap.parse_args()
    if args.launches < 50:
        sys.exit("metrics_bench: --launches must be at least 50")
    if not torch.cuda.is_available():
        sys.exit("metrics_bench: no GPU -- this tool measures on an MI355X and has no other mode")
    torch.cuda.set_device(0)
    only = set(args.only.split(","))
    if not only or only - {"kernel", "grad", "eval_gop"}:
        sys.exit("metrics_bench: --only takes kernel, grad, eval_gop")
    res = {"device": torch.cuda.get_device_name(0)}
    if "kernel" in only:
        res["kernel"] = [time_kernel((1, 3, 1080, 1920), args.launches), time_kernel((8, 3, 1080, 1920), args.launches)]
    if "grad" in only:
        res["grad"] = [time_grad((16, 3, 256, 256), args.launches), time_grad((1, 3, 1080, 1920), args.launches)]
    if "eval_gop" in only:
        res["eval_gop"] = time_eval(args.passes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
