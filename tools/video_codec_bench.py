"""What the stand-alone sequence codec costs per frame, beside the evaluation loop it replaces for coding, and the two frame kernels beside
the two-pass compositions they fold.

    python tools/video_codec_bench.py [--frames 24] [--gop 12] [--concurrent 8] [--reps 5] [--launches 60]
                                      [--part all|baseline] [--baseline FILE] [--out profiles/video_codec.json] [--state-hash]

Workload: `--frames` synthetic 1080p frames (tools/sequence_bench.py's) quantised to a raw 4:2:0 file at 8 and at 10 bits, gop `--gop`,
the models of `bench.py --config eval` (mbt2018 quality 4, SpatioTemporalPriorModel_Res, closed-form weights).

1. sequence, per bit depth: video.encode_sequence (file out, no decoder), evaluation.eval_sequence (encode + decode per frame,
   with_msssim=False) and video.decode_sequence (planar 4:2:0 out), one after the other `--reps` times after a warm-up pass of each:
   HIP events around each pass (the host coder's time lies between them), seconds per frame as median with the 10th and 90th percentile.
2. kernels, per bit depth, one 1080p frame in 1088 x 1920: functional.yuv420_to_rgb_padded beside bitstream.pad(functional.yuv420_to_rgb),
   functional.rgb_window_to_yuv420 beside functional.rgb_to_yuv420(bitstream.crop(.).contiguous()), alternating call by call, `--launches`
   times: microseconds as median / p10 / p90, and the bytes the FUSED pass must move (from the shapes: every input read once, every output
   written once) over each route's median, in GB/s.  The buffers are the same on every call and fit the Infinity Cache: a cache-warm rate.

`--part baseline` runs only what exists without video.py -- eval_sequence and the two-pass compositions -- so that the same file, copied
into a checkout of the parent commit, measures the parent in the same session; `--baseline FILE` puts that run's JSON under "parent".

`--state-hash` measures the opt-in per-frame state hashes instead and writes (merges) the keys "latent" and "kernel" of
profiles/state_hash.json (tools/pixel_codec_bench.py --state-hash writes "pixel"): at 8 bits, alternating, `--reps` passes each --
encode_sequence without and with state_hash=True, decode_sequence of the un-hashed file, of the hashed file with and without verify, and
verify_sequence (latents only), every repeat listed so that the spread shows; and functional.state_hash alone at [1,192,68,120]
channels-last and [1,3,1088,1920] planar beside a device-to-device copy of the same bytes, microseconds per call over batches of 50 calls.
With `--part baseline` only encode_sequence and decode_sequence run, without the new keywords: the parent commit's figures by the same
tool in the same session (`--baseline FILE` stores them under "latent"/"parent").
Nothing is gated on these numbers.  Needs an MI355X: without a GPU it fails, it measures nothing on a CPU.
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

H, W = 1080, 1920


def _pct(values):
    v = sorted(values)
    return {"median": statistics.median(v), "p10": v[int(0.1 * (len(v) - 1))], "p90": v[int(round(0.9 * (len(v) - 1)))]}


def _models(dev):
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    from spatiotemporalentropymodel_amd.zoo import models
    imodel = closed_form_fill_(models["mbt2018"](quality=4)).to(dev).eval()
    imodel.update(force=True)
    stem = closed_form_fill_(SpatioTemporalPriorModel_Res()).to(dev).eval()
    stem.update(force=True)
    return imodel, stem


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


def time_sequence(imodel, stem, bits, args, tmp, baseline_only):
    from spatiotemporalentropymodel_amd import data, evaluation
    dev = torch.device("cuda", 0)
    raw = os.path.join(tmp, f"src{bits}.yuv")
    _write_source(raw, args.frames, bits, dev)
    seq = data.YUVSequence(raw, W, H, bit_depth=bits, device=dev)
    coded, out = os.path.join(tmp, f"seq{bits}.stmv"), os.path.join(tmp, f"dec{bits}.yuv")
    routes = {"eval_sequence": lambda: evaluation.eval_sequence(imodel, stem, list(seq), gop=args.gop, concurrent_gops=args.concurrent, with_msssim=False)}
    if not baseline_only:
        from spatiotemporalentropymodel_amd import video
        routes = {"encode_sequence": lambda: video.encode_sequence(imodel, stem, seq, coded, gop=args.gop, concurrent_gops=args.concurrent),
                  **routes,
                  "decode_sequence": lambda: video.decode_sequence(imodel, stem, coded, write_to=out, concurrent_gops=args.concurrent, return_frames=False)}
    for fn in routes.values():                                   # warm-up: every kernel, both decoder forms, the persistent decoder's self-check
        fn()
    times = {k: [] for k in routes}
    for _ in range(args.reps):
        for k, fn in routes.items():                             # alternating
            times[k].append(_timed(fn) / args.frames)
    res = {"bits": bits, "frames": args.frames, "gop": args.gop, "concurrent_gops": args.concurrent, "reps": args.reps,
           "seconds_per_frame": {k: _pct(v) for k, v in times.items()}}
    if not baseline_only:
        ref = evaluation.eval_sequence(imodel, stem, list(seq), gop=args.gop, concurrent_gops=args.concurrent, with_msssim=False, write_to=out + ".ref")
        from spatiotemporalentropymodel_amd import bitstream, video
        blob = open(coded, "rb").read()
        recs = [bitstream.read_frame(io.BytesIO(blob[a:b]))[3] for a, b in video.record_ranges(blob, args.frames)]
        res["same_strings_as_eval_sequence"] = recs == [f["strings"] for f in ref["frames"]]
        res["same_yuv_as_eval_sequence"] = open(out, "rb").read() == open(out + ".ref", "rb").read()
        res["file_bytes"] = len(blob)
        m = res["seconds_per_frame"]
        res["eval_sequence_over_encode_sequence"] = m["eval_sequence"]["median"] / m["encode_sequence"]["median"]
    return res


def time_state_hash_sequence(imodel, stem, args, tmp, baseline_only):
    from spatiotemporalentropymodel_amd import data, video
    dev = torch.device("cuda", 0)
    raw = os.path.join(tmp, "src8.yuv")
    _write_source(raw, args.frames, 8, dev)
    seq = data.YUVSequence(raw, W, H, bit_depth=8, device=dev)
    plain, hashed, out = os.path.join(tmp, "plain.stmv"), os.path.join(tmp, "hashed.stmv"), os.path.join(tmp, "dec.yuv")
    kw = dict(gop=args.gop, concurrent_gops=args.concurrent)
    routes = {"encode_sequence": lambda: video.encode_sequence(imodel, stem, seq, plain, **kw),
              "decode_sequence": lambda: video.decode_sequence(imodel, stem, plain, write_to=out, concurrent_gops=args.concurrent, return_frames=False)}
    if not baseline_only:
        routes.update({
            "encode_sequence_state_hash": lambda: video.encode_sequence(imodel, stem, seq, hashed, state_hash=True, **kw),
            "decode_sequence_verified": lambda: video.decode_sequence(imodel, stem, hashed, write_to=out, concurrent_gops=args.concurrent,
                                                                      return_frames=False),
            "decode_sequence_verify_false": lambda: video.decode_sequence(imodel, stem, hashed, write_to=out, concurrent_gops=args.concurrent,
                                                                          return_frames=False, verify=False),
            "verify_sequence": lambda: video.verify_sequence(imodel, stem, hashed, concurrent_gops=args.concurrent)})
    for fn in routes.values():
        fn()
    times = {k: [] for k in routes}
    for _ in range(args.reps):
        for k, fn in routes.items():                             # alternating
            times[k].append(_timed(fn) / args.frames)
    res = {"bits": 8, "frames": args.frames, "gop": args.gop, "concurrent_gops": args.concurrent, "reps": args.reps,
           "seconds_per_frame": {k: dict(_pct(v), repeats=v) for k, v in times.items()}}
    if not baseline_only:
        a, b = open(plain, "rb").read(), open(hashed, "rb").read()
        res["records_equal_the_unhashed_files"] = b[5:len(a)] == a[5:] and len(b) == len(a) + 8 * args.frames
        res["verify_report"] = video.verify_sequence(imodel, stem, hashed, concurrent_gops=args.concurrent)
        m = {k: v["median"] for k, v in res["seconds_per_frame"].items()}
        res["encode_with_hashes_over_without"] = m["encode_sequence_state_hash"] / m["encode_sequence"]
        res["decode_verified_over_unhashed"] = m["decode_sequence_verified"] / m["decode_sequence"]
        res["verify_sequence_over_decode_sequence"] = m["verify_sequence"] / m["decode_sequence"]
    return res


def time_state_hash_kernel(rounds=12, batch=50):
    """functional.state_hash beside dst.copy_(src) of the same tensor, alternating batches of `batch` calls between two events"""
    from spatiotemporalentropymodel_amd import functional as F
    dev = torch.device("cuda", 0)
    rows = []
    for name, t in (("y_hat [1,192,68,120] channels-last", torch.randn(1, 192, 68, 120, device=dev).contiguous(memory_format=torch.channels_last)),
                    ("x_hat [1,3,1088,1920] planar", torch.rand(1, 3, 1088, 1920, device=dev))):
        dst, out = torch.empty_like(t), torch.empty(1, dtype=torch.int64, device=dev)
        fns = {"state_hash": lambda: F.state_hash(t, out=out), "copy_d2d": lambda: dst.copy_(t)}
        for fn in fns.values():
            for _ in range(batch):
                fn()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(_timed(lambda: [fn() for _ in range(batch)]) / batch * 1e6)
        nbytes = 4 * t.numel()
        rows.append({"tensor": name, "bytes": nbytes, "calls_per_batch": batch, "batches": rounds,
                     "microseconds_per_call": {k: _pct(v) for k, v in times.items()},
                     "GB_per_s_read": {k: nbytes / (_pct(v)["median"] * 1e-6) / 1e9 for k, v in times.items()},
                     "note": "the copy also writes the same bytes; both include the host's launch path (the hash: two launches and a workspace allocation)"})
    return rows


def state_hash_main(args):
    dev = torch.device("cuda", 0)
    base = args.part == "baseline"
    res = {"device": torch.cuda.get_device_name(0), "part": args.part,
           "workload": f"{args.frames} synthetic {W}x{H} frames at 8 bits, gop {args.gop}, models of bench.py --config eval"}
    with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
        imodel, stem = _models(dev)
        res.update(time_state_hash_sequence(imodel, stem, args, tmp, base))
        kernel = None if base else time_state_hash_kernel()
    if args.baseline:
        with open(args.baseline) as f:
            res["parent"] = json.load(f)
    merged = {}
    if not base and os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged = res if base else dict(merged, latent=res, kernel=kernel)
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


def time_kernels(bits, launches, baseline_only):
    from spatiotemporalentropymodel_amd import bitstream, functional as F
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(bits)
    dt, sb = (torch.uint8, 1) if bits == 8 else (torch.uint16, 2)
    y, u, v = (torch.randint(0, 1 << bits, s, device=dev, generator=gen, dtype=torch.int32).to(dt) for s in ((1, H, W), (1, H // 2, W // 2), (1, H // 2, W // 2)))
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    x = torch.rand((1, 3, Hp, Wp), device=dev, generator=gen)
    ingest = {"two_pass": lambda: bitstream.pad(F.yuv420_to_rgb(y, u, v, bits, "bilinear", True), 64)}
    emit = {"two_pass": lambda: F.rgb_to_yuv420(bitstream.crop(x, (H, W)).contiguous(), bits)}
    if not baseline_only:
        ingest["fused"] = lambda: F.yuv420_to_rgb_padded(y, u, v, bits, "bilinear", True, multiple=64)
        emit["fused"] = lambda: F.rgb_window_to_yuv420(x, (H, W), bits)
    rows = []
    for name, fns, nbytes in (("ingest", ingest, 1.5 * sb * H * W + 12 * Hp * Wp), ("emit", emit, 12 * H * W + 1.5 * sb * H * W)):
        t = _alternate(fns, launches)
        rows.append({"kernel": name, "bits": bits, "frame": [Hp, Wp], "image": [H, W], "launches": launches, "bytes_of_the_fused_pass": nbytes,
                     "microseconds": t, "GB_per_s_of_those_bytes": {k: nbytes / (d["median"] * 1e-6) / 1e9 for k, d in t.items()}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--gop", type=int, default=12)
    ap.add_argument("--concurrent", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--part", default="all", choices=("all", "baseline"))
    ap.add_argument("--baseline", default=None, help="JSON of a `--part baseline` run on the parent commit, stored under \"parent\"")
    ap.add_argument("--state-hash", action="store_true", help="measure the per-frame state hashes into profiles/state_hash.json instead")
    ap.add_argument("--out", default=None, help="default: profiles/video_codec.json, with --state-hash profiles/state_hash.json")
    args = ap.parse_args()
    args.out = args.out or os.path.join(REPO, "profiles", "state_hash.json" if args.state_hash else "video_codec.json")
    if not torch.cuda.is_available():
        sys.exit("video_codec_bench: no GPU -- this tool measures on an MI355X and has no other mode")
    torch.cuda.set_device(0)
    if args.state_hash:
        return state_hash_main(args)
    dev = torch.device("cuda", 0)
    base = args.part == "baseline"
    res = {"device": torch.cuda.get_device_name(0), "part": args.part,
           "workload": f"{args.frames} synthetic {W}x{H} frames, gop {args.gop}, models of bench.py --config eval, with_msssim=False"}
    with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
        imodel, stem = _models(dev)
        res["sequence"] = [time_sequence(imodel, stem, bits, args, tmp, base) for bits in (8, 10)]
        res["kernels"] = [r for bits in (8, 10) for r in time_kernels(bits, args.launches, base)]
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
