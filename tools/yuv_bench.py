"""Time of the two YUV 4:2:0 kernels (stem_yuv420_to_rgb, stem_rgb_to_yuv420; csrc/yuv.hip) beside the torch composition of the same
steps on the same GPU (what a user had before: the reference's transforms as eager device operations).

    python tools/yuv_bench.py [--launches 60] [--out profiles/yuv_bench.json]

Shapes [1,.,1080,1920] and [16,.,256,256], 8- and 10-bit.  Per shape and direction: HIP events around every call after a warm-up,
the two routes ALTERNATING call by call, the median of `--launches` (>= 50).  The timed region of the HIP route is the
functional.* call: the Python wrapper, its output allocations (torch's caching allocator) and the launch(es).  Bytes moved are
computed from the shapes (every plane read or written once) and reported over that time relative to 6.3 TB/s; the buffers (28 MB
at 1080p) are the same on every call and fit the 256 MB Infinity Cache, so this is a CACHE-WARM rate, not an HBM efficiency.  The
torch route (a 3 x 3 matrix over the channel axis, interpolate / avg_pool2d, round(clamp(.) * peak)) forms no sums of squared
errors; the HIP time includes them in the "hip_sse" columns.

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

HBM_ACHIEVABLE = 6.3e12        # bytes/s a streaming kernel reaches on an MI355X (8 TB/s peak)
SHAPES = [(1, 1080, 1920), (16, 256, 256)]
# BT.709, full range, as matrices: [y, cb - 0.5, cr - 0.5] = FROM_RGB @ [r, g, b] and its inverse
_W = torch.tensor([0.2126, 0.7152, 0.0722], dtype=torch.float64)
FROM_RGB = torch.stack((_W, (torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64) - _W) / (2 * (1 - _W[2])),
                        (torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64) - _W) / (2 * (1 - _W[0]))))
TO_RGB = torch.linalg.inv(FROM_RGB)
HALF = torch.tensor([0.0, 0.5, 0.5])


def torch_to_rgb(y, u, v, peak, to_rgb, half):
    """eager device torch: normalise, bilinear x2 chroma, one 3 x 3 matrix over the channel axis, clamp"""
    up = [torch.nn.functional.interpolate(c.unsqueeze(1).float(), scale_factor=2, mode="bilinear", align_corners=False) for c in (u, v)]
    ycc = torch.cat([y.unsqueeze(1).float()] + up, dim=1) / peak - half.view(1, 3, 1, 1)
    return torch.einsum("oc,nchw->nohw", to_rgb, ycc).clamp_(0, 1)


def torch_to_yuv(x, peak, dtype, from_rgb, half):
    """eager device torch: one 3 x 3 matrix, 2 x 2 chroma mean, quantise"""
    ycc = torch.einsum("oc,nchw->nohw", from_rgb, x) + half.view(1, 3, 1, 1)
    planes = (ycc[:, 0], *torch.nn.functional.avg_pool2d(ycc[:, 1:], 2).unbind(1))
    return tuple(torch.round(p.clamp(0, 1) * peak).to(dtype) for p in planes)


def alternate(fns, launches, warmup=10):
    """median / min / p90 (microseconds) of each callable, timed with events, alternating call by call"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)] for k in fns}
    for i in range(launches):
        for k, fn in fns.items():
            a, b = ev[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    out = {}
    for k in fns:
        us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[k])
        out[k] = {"median_us": statistics.median(us), "min_us": us[0], "p90_us": us[int(0.9 * (launches - 1))]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/yuv_bench.py measures on an MI355X; no GPU found")
    from spatiotemporalentropymodel_amd import functional as F
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    to_rgb, from_rgb, half = TO_RGB.float().to(dev), FROM_RGB.float().to(dev), HALF.to(dev)
    rows = []
    for B, H, W in SHAPES:
        for bits in (8, 10):
            peak, dt, sb = float((1 << bits) - 1), (torch.uint8 if bits == 8 else torch.int16), (1 if bits == 8 else 2)
            planes = tuple(torch.randint(0, 1 << bits, s, device=dev, generator=gen, dtype=torch.int32).to(dt)
                           for s in ((B, H, W), (B, H // 2, W // 2), (B, H // 2, W // 2)))
            hip_planes = planes if bits == 8 else tuple(p.view(torch.uint16) for p in planes)
            x = torch.rand((B, 3, H, W), device=dev, generator=gen)
            src = F.rgb_to_yuv420(x, bit_depth=bits)
            npix = B * H * W
            t = alternate({"hip": lambda: F.yuv420_to_rgb(*hip_planes, bit_depth=bits), "torch": lambda: torch_to_rgb(*planes, peak, to_rgb, half)}, args.launches)
            nbytes = npix * (1.5 * sb + 12)
            rows.append({"kernel": "stem_yuv420_to_rgb", "shape": [B, H, W], "bits": bits, "bytes_from_shapes": nbytes, **{f"{k}_{m}": v for k, d in t.items() for m, v in d.items()},
                         "hip_cache_warm_bytes_per_s_over_6.3TBps": nbytes / (t["hip"]["median_us"] * 1e-6) / HBM_ACHIEVABLE})
            t = alternate({"hip": lambda: F.rgb_to_yuv420(x, bit_depth=bits), "hip_sse": lambda: F.rgb_to_yuv420(x, bit_depth=bits, source=src),
                           "torch": lambda: torch_to_yuv(x, peak, dt, from_rgb, half)}, args.launches)
            nbytes = npix * (12 + 1.5 * sb)
            rows.append({"kernel": "stem_rgb_to_yuv420", "shape": [B, H, W], "bits": bits, "bytes_from_shapes": nbytes, **{f"{k}_{m}": v for k, d in t.items() for m, v in d.items()},
                         "hip_cache_warm_bytes_per_s_over_6.3TBps": nbytes / (t["hip"]["median_us"] * 1e-6) / HBM_ACHIEVABLE})
            # the two routes agree (the torch one is fp32: a step of difference next to a half-integer)
            a, b = F.yuv420_to_rgb(*hip_planes, bit_depth=bits), torch_to_rgb(*planes, peak, to_rgb, half)
            rows[-2]["max_abs_diff_vs_torch"] = float((a - b).abs().max())
            q, r = F.rgb_to_yuv420(x, bit_depth=bits)[0], torch_to_yuv(x, peak, dt, from_rgb, half)[0]
            rows[-1]["y_samples_differing_from_torch"] = int((q.view(dt) != r).sum())
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "launches": args.launches, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
