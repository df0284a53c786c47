#!/usr/bin/env python3
"""configs[3]-shaped codec timing: one 1080p P-frame latent (y [1,192,68,120]) through compress / decompress.

    python tools/codec_bench.py                       raster order (the reference's), one frame
    python tools/codec_bench.py --order wavefront     the wavefront symbol order (codec.wave_order)
    python tools/codec_bench.py --order both --passes 3 --chains 8 --json profiles/wave_decode.json
                                                      both orders in ONE process on the same frame, alternating passes, for one chain
                                                      and for `--chains` chains through the *_each entry points; the figures (per-frame
                                                      decode time, time per sequential step, the host coder's share) go to the file

The host coder's share is measured where it can be isolated: the frame's y string decoded by the host library alone, with the indexes
the encoder produced, in the chunks the decoder asks for (M symbols per position in raster order, np(t) * M per step in wavefront
order).  STEM_AR_PROFILE=1 makes the lockstep and wavefront loops print their own launch / wait / host split per step.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from spatiotemporalentropymodel_amd import codec  # noqa: E402
from spatiotemporalentropymodel_amd.entropy_models import RansDecoder  # noqa: E402
from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res  # noqa: E402
from spatiotemporalentropymodel_amd.weights import closed_form_fill_  # noqa: E402

H, W, M = 68, 120, 192


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _host_coder_seconds(m, string, order, record):
    """the host library alone on this string: one decode call per sequential step of `order`, with the encoder's indexes"""
    idx = record[order]
    sizes = [M] * (H * W) if order == "raster" else [int(n) * M for n in codec.wave_order(H, W)[1] if n]
    tables = m.gaussian_conditional.host_tables()
    dec = RansDecoder()
    dec.set_stream(string)
    chunks = np.split(idx, np.cumsum(sizes)[:-1])
    t0 = time.perf_counter()
    for c in chunks:
        dec.decode_stream_np(c, tables)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--order", choices=("raster", "wavefront", "both"), default="raster")
    ap.add_argument("--passes", type=int, default=1, help="timed passes per order (alternating when --order both)")
    ap.add_argument("--chains", type=int, default=0, help="also time this many chains through stem_compress_each / stem_decompress_each")
    ap.add_argument("--json", default=None, help="write the figures to this file")
    args = ap.parse_args()
    orders = ("raster", "wavefront") if args.order == "both" else (args.order,)

    m = SpatioTemporalPriorModel_Res()
    closed_form_fill_(m)
    m = m.cuda().eval()
    m.update(force=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    n = max(1, args.chains)
    y_cond = torch.randn(n, M, H, W, device="cuda", generator=g) * 3
    y_cur = y_cond + torch.randn(n, M, H, W, device="cuda", generator=g) * 2
    one = (y_cur[:1].contiguous(), y_cond[:1].contiguous())
    kw = {o: ({} if o == "raster" else {"order": o}) for o in orders}

    # the indexes each order's host coder sees (for the host-only timing), recorded from the encoder's own call
    record = {}

    class Recorder(codec.BufferedRansEncoder):
        def encode_with_indexes(self, symbols, indexes, tables):
            record[Recorder.order] = np.ascontiguousarray(np.asarray(indexes).reshape(-1), dtype=np.int32)
            super().encode_with_indexes(symbols, indexes, tables)

    res = {"frame": f"1080p P-frame latent [1,{M},{H},{W}]", "steps": {"raster": H * W, "wavefront": int((codec.wave_order(H, W)[1] > 0).sum())},
           "passes": args.passes, "one_chain": {}, "chains": {}}
    with torch.no_grad():
        enc = {}
        plain, codec.BufferedRansEncoder = codec.BufferedRansEncoder, Recorder
        try:
            for o in orders:                                   # warm-up: first use of every kernel, the persistent route's self-check
                Recorder.order = o
                enc[o] = m.compress(*one, **kw[o])
        finally:
            codec.BufferedRansEncoder = plain
        for o in orders:
            m.decompress(enc[o]["strings"], enc[o]["shape"], one[1], **kw[o])
        t_enc, t_dec = {o: [] for o in orders}, {o: [] for o in orders}
        outs = {}
        for _ in range(args.passes):
            for o in orders:                                   # alternating passes: both orders see the same clocks
                enc[o], t = _timed(lambda: m.compress(*one, **kw[o]))
                t_enc[o].append(t)
                out, t = _timed(lambda: m.decompress(enc[o]["strings"], enc[o]["shape"], one[1], **kw[o]))
                outs[o] = out["y_hat"] if isinstance(out, dict) else out
                t_dec[o].append(t)
        if len(orders) == 2:
            assert torch.equal(outs["raster"], outs["wavefront"]), "the two orders decode to different latents"
            assert enc["raster"]["strings"][1] == enc["wavefront"]["strings"][1]
        for o in orders:
            nbytes = len(enc[o]["strings"][0][0]) + len(enc[o]["strings"][1][0])
            host = min(_host_coder_seconds(m, enc[o]["strings"][0][0], o, record) for _ in range(max(1, args.passes)))
            dec = min(t_dec[o])
            res["one_chain"][o] = {"compress_s": min(t_enc[o]), "decompress_s": dec, "decompress_all_s": t_dec[o], "bytes": nbytes,
                                   "us_per_step": 1e6 * dec / res["steps"][o], "host_coder_s": host, "host_coder_share": host / dec}
            print("1080p P-frame latent, %s order: compress %.3f s, decompress %.3f s (%.1f us per step over %d steps; host coder alone %.3f s = %.0f %%), "
                  "%d bytes (%.3f bpp)" % (o, min(t_enc[o]), dec, 1e6 * dec / res["steps"][o], res["steps"][o], host, 100 * host / dec, nbytes,
                                           8 * nbytes / (1088 * 1920)))
        if args.chains > 1:
            curs, conds = [y_cur[i:i + 1].contiguous() for i in range(n)], [y_cond[i:i + 1].contiguous() for i in range(n)]
            encs, t_dec = {}, {o: [] for o in orders}
            for o in orders:
                encs[o] = codec.stem_compress_each(m, curs, conds, **kw[o])
                codec.stem_decompress_each(m, [e["strings"] for e in encs[o]], [e["shape"] for e in encs[o]], conds, **kw[o])
            for _ in range(args.passes):
                for o in orders:
                    outs[o], t = _timed(lambda: codec.stem_decompress_each(m, [e["strings"] for e in encs[o]], [e["shape"] for e in encs[o]], conds, **kw[o]))
                    t_dec[o].append(t)
            if len(orders) == 2:
                assert all(torch.equal(a, b) for a, b in zip(outs["raster"], outs["wavefront"]))
            for o in orders:
                dec = min(t_dec[o])
                res["chains"][o] = {"chains": n, "decompress_s": dec, "decompress_all_s": t_dec[o], "decompress_s_per_frame": dec / n}
                print("%d chains through stem_decompress_each, %s order: %.3f s = %.3f s per frame" % (n, o, dec, dec / n))
    print("reference (survey container, torch CPU): 13 s + 39 s per frame (SURVEY.md 3.2)")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
