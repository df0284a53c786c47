"""What the pixel-domain sequence codec costs per frame, beside the evaluation loop it replaces for coding, and its two per-frame kernels
beside the compositions they fold.

    python tools/pixel_codec_bench.py [--frames 12] [--gop 12] [--reps 3] [--launches 60]
                                      [--part all|baseline] [--baseline FILE] [--out profiles/pixel_codec.json] [--state-hash]

Workload: `--frames` synthetic 1080p frames quantised to a raw 4:2:0 file at 8 and at 10 bits, gop `--gop`, stem_roi_i + stem_roi on
closed-form weights (convolutions scaled by 0.7, as the tests' fixtures), four feathered rectangles per frame over the level 0.3.

1. sequence, per bit depth: video_pixel.encode_sequence (rois=, file out, no decoder), evaluation.eval_gop_pixel (encode + forward +
   decode per frame with the same maps as host tensors, with_msssim=False) and video_pixel.decode_sequence (planar 4:2:0 out), one after
   the other `--reps` times after a warm-up pass of each: HIP events around each pass (the host coder's time lies between them), seconds
   per frame as median with the 10th and 90th percentile.
2. kernels, one 1080p frame in 1088 x 1920, alternating call by call, `--launches` times: functional.rgb_window_recondition with planes
   beside bitstream.pad(bitstream.crop(x)) + functional.rgb_window_to_yuv420 (per bit depth), and functional.roi_map_padded beside a
   ready host map through evaluation.quality_map + the copy to the device + bitstream.pad (the host route is not charged for rasterising).
   Microseconds as median / p10 / p90, and the bytes the FUSED pass must move (from the shapes: recondition reads the window once and
   writes the border and the planes once; the rasteriser writes the map once) over each route's median, in GB/s.  The buffers are the
   same on every call and fit the Infinity Cache: a cache-warm rate.

`--part baseline` runs only what exists without video_pixel.py -- eval_gop_pixel and the compositions -- so that the same file, copied into
a checkout of the parent commit, measures the parent in the same session; `--baseline FILE` puts that run's JSON under "parent".

`--state-hash` measures the opt-in per-frame state hashes instead and writes (merges) the key "pixel" of profiles/state_hash.json
(tools/video_codec_bench.py --state-hash writes "latent" and "kernel"): at 8 bits, alternating, `--reps` passes each -- encode_sequence
without and with state_hash=True, decode_sequence of the un-hashed file, of the hashed file with and without verify, and verify_sequence,
every repeat listed so that the spread shows.  With `--part baseline` only encode_sequence and decode_sequence run, without the new
keywords: the parent commit's figures by the same tool in the same session (`--baseline FILE` stores them under "pixel"/"parent").
Nothing is gated on these numbers.  Needs an MI355X: without a GPU it fails, it measures nothing on a CPU.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 1080, 1920
LEVEL = 0.3


def _pct(values):
    v = sorted(values)
    return {"median": statistics.median(v), "p10": v[int(0.1 * (len(v) - 1))], "p90": v[int(round(0.9 * (len(v) - 1)))]}


def _models(dev):
    from spatiotemporalentropymodel_amd.models import stem_roi, stem_roi_i
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_scaled_
    out = []
    for cls, tag in ((stem_roi_i, "roi_i"), (stem_roi, "roi_p")):
        m = closed_form_fill_scaled_(cls(), tag, 0.7).to(dev).eval()
        m.update(force=True)
        out.append(m)
    return out


def _boxes(t):
    """four rectangles of frame t: a large feathered one that moves, one that leaves the frame, a hard-edged one, one below the level"""
    return [(300 + 16 * t, 200, 1100 + 16 * t, 800, 0.9, 32), (1500, 700 - 8 * t, 2000, 1200, 0.65, 15), (40, 40, 240, 160, 1.0),
            (900, 500, 1000, 600, 0.1, 4)]


def _host_map(boxes):
    """the same map on the host, in float32 numpy (the statement of include/stem_roiio.h), for the routes that take host tensors"""
    out = np.full((H, W), np.float32(LEVEL), dtype=np.float32)
    for x0, y0, x1, y1, value, *rest in boxes:
        feather = rest[0] if rest else 0
        ra, rb, ca, cb = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
        r, c = np.arange(ra, rb)[:, None], np.arange(ca, cb)[None, :]
        d = np.minimum(np.minimum(c - x0, x1 - 1 - c), np.minimum(r - y0, y1 - 1 - r))
        t = (d + 1).astype(np.float32) / np.float32(feather + 1)
        v = out[ra:rb, ca:cb]
        out[ra:rb, ca:cb] = np.where(d >= feather, np.float32(value), v + (np.float32(value) - v) * t)
    return torch.from_numpy(out)


def _write_source(path, n_frames, bits, dev):
    from spatiotemporalentropymodel_amd import data
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    for t in range(n_frames):
        x = torch.stack([0.5 + 0.4 * torch.sin((xx + 3 * t) / (40.0 + 10 * c)) * torch.cos((yy + t) / (55.0 - 5 * c)) for c in range(3)])
        data.write_yuv420(path, x, bit_depth=bits, append=t > 0)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def time_sequence(model_i, model_p, bits, args, tmp, baseline_only):
    from spatiotemporalentropymodel_amd import data, evaluation
    dev = torch.device("cuda", 0)
    raw = os.path.join(tmp, f"src{bits}.yuv")
    _write_source(raw, args.frames, bits, dev)
    seq = data.YUVSequence(raw, W, H, bit_depth=bits, device=dev)
    rois = [_boxes(t) for t in range(args.frames)]
    maps = [_host_map(b) for b in rois]
    coded, out = os.path.join(tmp, f"seq{bits}.stpx"), os.path.join(tmp, f"dec{bits}.yuv")
    routes = {"eval_gop_pixel": lambda: evaluation.eval_gop_pixel(model_i, model_p, seq, qmaps=maps, gop=args.gop, with_msssim=False, roi_weight=False)}
    if not baseline_only:
        from spatiotemporalentropymodel_amd import video_pixel
        routes = {"encode_sequence": lambda: video_pixel.encode_sequence(model_i, model_p, seq, coded, rois=rois, level=LEVEL, gop=args.gop),
                  **routes,
                  "decode_sequence": lambda: video_pixel.decode_sequence(model_i, model_p, coded, write_to=out, return_frames=False)}
    for fn in routes.values():                                   # warm-up: every kernel and shape once
        fn()
    times = {k: [] for k in routes}
    for _ in range(args.reps):
        for k, fn in routes.items():                             # alternating
            times[k].append(_timed(fn) / args.frames)
    res = {"bits": bits, "frames": args.frames, "gop": args.gop, "reps": args.reps, "seconds_per_frame": {k: _pct(v) for k, v in times.items()}}
    if not baseline_only:
        from spatiotemporalentropymodel_amd import functional as F
        from spatiotemporalentropymodel_amd import video, video_pixel
        ref = evaluation.eval_gop_pixel(model_i, model_p, seq, qmaps=maps, gop=args.gop, with_msssim=False, roi_weight=False)
        blob = open(coded, "rb").read()
        hdr = video_pixel.FileHeader.unpack(blob)
        ranges = video_pixel.record_ranges(blob, hdr.frames, video_pixel.HEADER_BYTES)
        recs = [video_pixel.read_record(blob, ranges[k], hdr, k, t)[1] for k, t in enumerate(hdr.types())]
        res["same_strings_as_eval_gop_pixel"] = recs == [f["strings"] for f in ref["frames"]]
        want = b"".join(video._planes_bytes(F.rgb_window_to_yuv420(f["x_hat"].contiguous(), (H, W), bits)) for f in ref["frames"])
        res["same_yuv_as_eval_gop_pixel"] = open(out, "rb").read() == want
        res["file_bytes"] = len(blob)
        res["bpp_ave"] = ref["bpp_ave"]
        m = res["seconds_per_frame"]
        res["eval_gop_pixel_over_encode_sequence"] = m["eval_gop_pixel"]["median"] / m["encode_sequence"]["median"]
    return res


def state_hash_main(args):
    from spatiotemporalentropymodel_amd import data, video_pixel
    dev = torch.device("cuda", 0)
    base = args.part == "baseline"
    res = {"device": torch.cuda.get_device_name(0), "part": args.part,
           "workload": f"{args.frames} synthetic {W}x{H} frames at 8 bits, gop {args.gop}, stem_roi_i + stem_roi on closed-form weights, four "
                       f"rectangles per frame over level {LEVEL}"}
    with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
        model_i, model_p = _models(dev)
        raw = os.path.join(tmp, "src8.yuv")
        _write_source(raw, args.frames, 8, dev)
        seq = data.YUVSequence(raw, W, H, bit_depth=8, device=dev)
        rois = [_boxes(t) for t in range(args.frames)]
        plain, hashed, out = os.path.join(tmp, "plain.stpx"), os.path.join(tmp, "hashed.stpx"), os.path.join(tmp, "dec.yuv")
        kw = dict(rois=rois, level=LEVEL, gop=args.gop)
        routes = {"encode_sequence": lambda: video_pixel.encode_sequence(model_i, model_p, seq, plain, **kw),
                  "decode_sequence": lambda: video_pixel.decode_sequence(model_i, model_p, plain, write_to=out, return_frames=False)}
        if not base:
            routes.update({
                "encode_sequence_state_hash": lambda: video_pixel.encode_sequence(model_i, model_p, seq, hashed, state_hash=True, **kw),
                "decode_sequence_verified": lambda: video_pixel.decode_sequence(model_i, model_p, hashed, write_to=out, return_frames=False),
                "decode_sequence_verify_false": lambda: video_pixel.decode_sequence(model_i, model_p, hashed, write_to=out, return_frames=False,
                                                                                    verify=False),
                "verify_sequence": lambda: video_pixel.verify_sequence(model_i, model_p, hashed)})
        for fn in routes.values():
            fn()
        times = {k: [] for k in routes}
        for _ in range(args.reps):
            for k, fn in routes.items():                         # alternating
                times[k].append(_timed(fn) / args.frames)
        res.update({"bits": 8, "frames": args.frames, "gop": args.gop, "reps": args.reps,
                    "seconds_per_frame": {k: dict(_pct(v), repeats=v) for k, v in times.items()}})
        if not base:
            a, b = open(plain, "rb").read(), open(hashed, "rb").read()
            res["records_equal_the_unhashed_files"] = b[5:len(a)] == a[5:] and len(b) == len(a) + 8 * args.frames
            res["verify_report"] = video_pixel.verify_sequence(model_i, model_p, hashed)
            m = {k: v["median"] for k, v in res["seconds_per_frame"].items()}
            res["encode_with_hashes_over_without"] = m["encode_sequence_state_hash"] / m["encode_sequence"]
            res["decode_verified_over_unhashed"] = m["decode_sequence_verified"] / m["decode_sequence"]
            res["verify_sequence_over_decode_sequence"] = m["verify_sequence"] / m["decode_sequence"]
    if args.baseline:
        with open(args.baseline) as f:
            res["parent"] = json.load(f)
    merged = {}
    if not base and os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged = res if base else dict(merged, pixel=res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    print(json.dumps(merged))


def _alternate(fns, launches, warmup=10):
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
    return {k: _pct([a.elapsed_time(b) * 1e3 for a, b in ev[k]]) for k in fns}


def time_kernels(launches, baseline_only):
    from spatiotemporalentropymodel_amd import bitstream, evaluation, functional as F
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    x = torch.rand((1, 3, Hp, Wp), device=dev, generator=gen)
    rows = []

    def row(name, bits, fns, nbytes):
        t = _alternate(fns, launches)
        rows.append({"kernel": name, "bits": bits, "frame": [Hp, Wp], "image": [H, W], "launches": launches, "bytes_of_the_fused_pass": nbytes,
                     "microseconds": t, "GB_per_s_of_those_bytes": {k: nbytes / (d["median"] * 1e-6) / 1e9 for k, d in t.items()}})

    for bits in (8, 10):
        sb = 1 if bits == 8 else 2

        def two_pass(bits=bits):
            y = bitstream.pad(bitstream.crop(x, (H, W)), 64)
            return y, F.rgb_window_to_yuv420(x, (H, W), bits)

        fns = {"two_pass": two_pass}
        if not baseline_only:
            fns["fused"] = lambda bits=bits: F.rgb_window_recondition(x, (H, W), bits)
        row("recondition", bits, fns, 12 * H * W + 12 * (Hp * Wp - H * W) + 1.5 * sb * H * W)
    boxes = _boxes(3)
    host = _host_map(boxes)
    fns = {"host_map": lambda: bitstream.pad(evaluation.quality_map(host, H, W).to(dev), 64)}
    if not baseline_only:
        fns["fused"] = lambda: F.roi_map_padded(boxes, (H, W), LEVEL, device=dev)
    row("roi_map", None, fns, 4 * Hp * Wp)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--gop", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--part", default="all", choices=("all", "baseline"))
    ap.add_argument("--baseline", default=None, help="JSON of a `--part baseline` run on the parent commit, stored under \"parent\"")
    ap.add_argument("--state-hash", action="store_true", help="measure the per-frame state hashes into profiles/state_hash.json instead")
    ap.add_argument("--out", default=None, help="default: profiles/pixel_codec.json, with --state-hash profiles/state_hash.json")
    args = ap.parse_args()
    args.out = args.out or os.path.join(REPO, "profiles", "state_hash.json" if args.state_hash else "pixel_codec.json")
    if not torch.cuda.is_available():
        sys.exit("pixel_codec_bench: no GPU -- this tool measures on an MI355X and has no other mode")
    torch.cuda.set_device(0)
    if args.state_hash:
        return state_hash_main(args)
    dev = torch.device("cuda", 0)
    base = args.part == "baseline"
    res = {"device": torch.cuda.get_device_name(0), "part": args.part,
           "workload": f"{args.frames} synthetic {W}x{H} frames, gop {args.gop}, stem_roi_i + stem_roi on closed-form weights, four rectangles per frame "
                       f"over level {LEVEL}, with_msssim=False"}
    with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
        model_i, model_p = _models(dev)
        res["sequence"] = [time_sequence(model_i, model_p, bits, args, tmp, base) for bits in (8, 10)]
        res["kernels"] = time_kernels(args.launches, base)
    if args.baseline:
        with open(args.baseline) as f:
            res["parent"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
