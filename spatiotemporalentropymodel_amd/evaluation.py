"""The evaluation loop of stem/evalSTEM.py (BASELINE configs[3]) as package functions.

    inference_iframe(imodel, x)                    stem/evalSTEM.py:34-89   (inferenceI_DVR)
    inference_pframe(imodel, stem, x, y_cond)      stem/evalSTEM.py:92-153  (inferenceP_DVR)
    eval_gop(imodel, stem, frames, gop=12)         the frame loop of evalDataset, stem/evalSTEM.py:180-216: frame index % GOP == 1
                                                   is an I frame coded by the image model's own compress / decompress, every other
                                                   frame a P frame conditioned on the previous frame's DECODED latents

Same order of operations, same returned keys, same arithmetic for bpp / PSNR as the script.  "ms-ssim": the script calls
`pytorch_msssim.ms_ssim(x, x_hat, data_range=1.0)` (:81, :147), a third-party package that is not in the reference tree (nor in this
image; unpinned in the reference's requirements): `ms_ssim` below restates the published algorithm (Wang, Simoncelli, Bovik 2003)
with that package's conventions.  PARITY UNPINNED for this one number -- no golden vector exists; tests/test_host_api.py checks it
against an independent scipy formulation and its defining properties.  It is a reporting metric outside the timed encode / decode
regions, computed on the host by default and by the HIP kernel on request: `with_msssim="device"` takes "ms-ssim" and "psnr" of a frame
from one stem_ms_ssim call (functional.ms_ssim, `ms_ssim_device` below; tests/test_hip_msssim.py holds it against float64); frames smaller than 161 pixels on a side have no five-scale MS-SSIM and report None.  One deliberate difference: the script's I frame runs
on the CPU and moves `y_conditioned` to the GPU for the P frames (:196-207); here everything stays on the models' device.
`yuv=True` (not in the script, which reads PNGs): every frame dictionary gains "psnr_y", "psnr_u", "psnr_v" and "psnr_yuv" =
(6 Y + U + V) / 8, the numbers video-coding papers tabulate, measured in the sample domain of the source: the decoded frame is
quantised to planar 4:2:0 at the source's bit depth and compared with the source's integer planes (`_yuv_metrics`); `write_to=`
appends each decoded frame to a raw .yuv file.  With yuv=False and no write_to nothing changes.
`order="wavefront"` (not in the script): the y strings hold their symbols in wavefront order (codec.wave_order) and decode in
W + 3(H-1) steps instead of H * W positions; reconstructions and PSNR are the raster run's, "bpp" is that of the frame's own strings.
The script's last line reads out_dec["entropy_params"], a key the reference model's decompress() does not return
(spatiotemporalpriors.py:1012 -> KeyError at :152 as shipped); the key is returned holding None.

Pinned by tests/golden/eval_gop.npz (tests/golden/make_golden.py:gen_eval_gop runs the reference's two functions themselves on
an I + 2 P chain) through tests/test_hip_codec.py::test_eval_gop_chain_matches_reference.
"""
from __future__ import annotations

import io
import math
import os
import time

import torch

from . import bitstream


def psnr(a: torch.Tensor, b: torch.Tensor) -> float:
    """stem/evalSTEM.py:29-31 (peak 1.0)"""
    mse = float(torch.mean((a.float() - b.float()) ** 2))
    return -10 * math.log10(mse)


_MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _gauss_window(size=11, sigma=1.5):
    c = torch.arange(size, dtype=torch.float64) - size // 2
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).float()


def _gauss_filter(x, win):
    """separable, 'valid' (no padding), one filter per channel"""
    C = x.shape[1]
    k = win.to(x.dtype)
    x = torch.nn.functional.conv2d(x, k.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return torch.nn.functional.conv2d(x, k.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)


def ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0):
    """Multi-scale structural similarity of two image batches [B,C,H,W] (host tensors; device tensors are copied): five scales,
    11-tap Gaussian window (sigma 1.5), K = (0.01, 0.03), the contrast-structure terms of scales 1-4 and the full SSIM of scale 5,
    each clamped at 0, raised to the published exponents and multiplied; 2x2 average pooling (odd sizes padded by one) between
    scales; mean over channels and batch.  None when the smaller side is <= 160 pixels (the fifth scale would be empty)."""
    x, y = x.detach().float().cpu(), y.detach().float().cpu()
    if min(x.shape[-2:]) <= (11 - 1) * 2 ** 4:
        return None
    win = _gauss_window()
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    terms = []
    for level in range(5):
        mu1, mu2 = _gauss_filter(x, win), _gauss_filter(y, win)
        s11 = _gauss_filter(x * x, win) - mu1 * mu1
        s22 = _gauss_filter(y * y, win) - mu2 * mu2
        s12 = _gauss_filter(x * y, win) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
        ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
        if level < 4:
            terms.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = [s % 2 for s in x.shape[2:]]
            x = torch.nn.functional.avg_pool2d(x, kernel_size=2, padding=pad)
            y = torch.nn.functional.avg_pool2d(y, kernel_size=2, padding=pad)
        else:
            terms.append(torch.relu(ssim_map.flatten(2).mean(-1)))
    w = torch.tensor(_MS_WEIGHTS).view(-1, 1, 1)
    return float(torch.prod(torch.stack(terms) ** w, dim=0).mean())


def ms_ssim_device(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0):
    """`ms_ssim` of two device batches by the HIP kernel (functional.ms_ssim): same contract -- a float, the mean over channels
    and batch, or None when the smaller side is <= 160 pixels.  One host read of the result."""
    from . import functional
    if min(x.shape[-2:]) <= (11 - 1) * 2 ** 4:
        return None
    return float(functional.ms_ssim(x.float(), y.float(), data_range)[0].double().mean())


def _metrics(x, x_hat, with_msssim):
    """("psnr", "ms-ssim") of one frame.  with_msssim: True = host `ms_ssim`, False = none, "device" = both numbers from one
    stem_ms_ssim call (its mean squared error is PSNR's), read back together; frames without a fifth scale fall to `psnr`."""
    if isinstance(with_msssim, str):
        if with_msssim != "device":
            raise ValueError(f'with_msssim is True, False or "device", got {with_msssim!r}')
        if min(x.shape[-2:]) > (11 - 1) * 2 ** 4:
            from . import functional
            ms, mse = functional.ms_ssim(x.float(), x_hat.float(), 1.0)
            ms, mse = torch.stack((ms.double().mean(), mse.double().mean())).tolist()
            return -10 * math.log10(mse), ms
        return psnr(x, x_hat), None
    return psnr(x, x_hat), (ms_ssim(x, x_hat, data_range=1.0) if with_msssim else None)


def _source_planes(frame):
    """the integer 4:2:0 planes a frame [3,h,w] came from and their bit depth: what data.YUVSequence attached to it, or, for a plain
    RGB tensor, the frame itself quantised at 8 bits"""
    planes = getattr(frame, "yuv_planes", None)
    if planes is not None:
        return planes, int(getattr(frame, "bit_depth", 8))
    from . import functional
    return functional.rgb_to_yuv420(frame.unsqueeze(0).float(), bit_depth=8), 8


def _psnr_int(sse, count, peak):
    """PSNR from an integer sum of squared sample errors; exactly zero error is +inf"""
    return float("inf") if sse == 0 else 10 * math.log10(peak * peak * count / sse)


def _yuv_metrics(frame, x_hat, yuv, write_to):
    """the yuv=True entries of one frame's dictionary (and the write_to side effect).  One stem_rgb_to_yuv420 call quantises the
    cropped x_hat [1,3,h,w] to the source's sample format and sums the squared integer differences against the source planes."""
    if not yuv and write_to is None:
        return {}
    from . import data, functional
    if not yuv:                                        # only the file is wanted: the source's depth, not its planes
        data.write_yuv420(write_to, x_hat, bit_depth=int(getattr(frame, "bit_depth", 8)), append=True)
        return {}
    planes, bit_depth = _source_planes(frame)
    y, u, v, sse = functional.rgb_to_yuv420(x_hat.float(), bit_depth=bit_depth, source=planes)
    if write_to is not None:
        data._write_planes(write_to, (y, u, v), append=True)
    sy, su, sv = sse[0].tolist()
    peak = (1 << bit_depth) - 1
    out = {"psnr_y": _psnr_int(sy, y.numel(), peak), "psnr_u": _psnr_int(su, u.numel(), peak), "psnr_v": _psnr_int(sv, v.numel(), peak)}
    out["psnr_yuv"] = (6 * out["psnr_y"] + out["psnr_u"] + out["psnr_v"]) / 8
    return out


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)


def _order_kw(order):
    """what compress / decompress are passed on top of the script's arguments: nothing for the reference's order"""
    from . import codec
    codec._check_order(order)
    return {} if order == "raster" else {"order": order}


def _bpp_terms(out_enc, out_forward, num_pixels):
    bpp = sum(len(s[0]) for s in out_enc["strings"]) * 8.0 / num_pixels
    est = {k: float(torch.log(v.float()).sum() / (-math.log(2) * num_pixels)) for k, v in out_forward["likelihoods"].items()}
    return bpp, est


@torch.no_grad()
def inference_iframe(model, x, with_msssim=True, yuv=False, write_to=None, order="raster"):
    """x: one image [3,h,w] in [0,1].  Pad to multiples of 64 (centred), compress + forward (the rate estimate), decompress, crop.
    `y_conditioned` is the DECODED latent of the padded image: what the next P frame is conditioned on.  yuv, write_to: `_yuv_metrics`;
    order: the symbol order of the y string ("raster" | "wavefront")."""
    okw = _order_kw(order)
    frame, x = x, x.unsqueeze(0)
    h, w = x.size(2), x.size(3)
    x_padded = bitstream.pad(x, 64)
    _sync(x)
    start = time.time()
    out_enc = model.compress(x_padded, **okw)
    out_forward = model(x_padded)
    _sync(x)
    enc_time = time.time() - start
    start = time.time()
    out_dec = model.decompress(out_enc["strings"], out_enc["shape"], **okw)
    _sync(x)
    dec_time = time.time() - start
    x_hat = bitstream.crop(out_dec["x_hat"], (h, w))
    num_pixels = x.size(0) * h * w
    bpp, est = _bpp_terms(out_enc, out_forward, num_pixels)
    quality = _metrics(x, x_hat, with_msssim)
    return {"y_conditioned": out_dec["y_hat"], "psnr": quality[0], "ms-ssim": quality[1], "bpp": bpp,
            "estimate_bpp": sum(est.values()),
            "estimate_y_bpp": est.get("y"), "estimate_z_bpp": est.get("z"), "y_bpp": len(out_enc["strings"][0][0]) * 8.0 / num_pixels,
            "z_bpp": len(out_enc["strings"][1][0]) * 8.0 / num_pixels, "encoding_time": enc_time, "decoding_time": dec_time,
            "out_forward": out_forward, "strings": out_enc["strings"], "shape": tuple(out_enc["shape"]), "x_hat": x_hat,
            **_yuv_metrics(frame, x_hat, yuv, write_to)}


@torch.no_grad()
def inference_pframe(imodel, stem, x, y_conditioned, with_msssim=True, yuv=False, write_to=None, order="raster"):
    """x: one frame [3,h,w]; y_conditioned: the previous frame's decoded latents.  encode = getY + forward + compress, decode =
    decompress + getX, timed as the script times them.  yuv, write_to: `_yuv_metrics`; order: as in `inference_iframe`."""
    okw = _order_kw(order)
    frame, x = x, x.unsqueeze(0)
    h, w = x.size(2), x.size(3)
    x_padded = bitstream.pad(x, 64)
    _sync(x)
    start = time.time()
    y_cur, _ = imodel.getY(x_padded)
    out_forward = stem(y_cur, y_conditioned)
    out_enc = stem.compress(y_cur, y_conditioned, **okw)
    _sync(x)
    enc_time = time.time() - start
    start = time.time()
    out_dec = stem.decompress(out_enc["strings"], out_enc["shape"], y_conditioned, **okw)
    y_hat = out_dec["y_hat"] if isinstance(out_dec, dict) else out_dec
    x_hat = imodel.getX(y_hat)
    _sync(x)
    dec_time = time.time() - start
    x_hat = bitstream.crop(x_hat, (h, w))
    num_pixels = x.size(0) * h * w
    bpp, est = _bpp_terms(out_enc, out_forward, num_pixels)
    quality = _metrics(x, x_hat, with_msssim)
    return {"y_conditioned": y_hat, "psnr": quality[0], "ms-ssim": quality[1], "bpp": bpp,
            "estimate_bpp": sum(est.values()),
            "estimate_y_bpp": est.get("y"), "estimate_z_bpp": est.get("z"), "y_bpp": len(out_enc["strings"][0][0]) * 8.0 / num_pixels,
            "z_bpp": len(out_enc["strings"][1][0]) * 8.0 / num_pixels, "encoding_time": enc_time, "decoding_time": dec_time,
            "entropy_params": out_dec.get("entropy_params") if isinstance(out_dec, dict) else None,
            "strings": out_enc["strings"], "shape": tuple(out_enc["shape"]), "x_hat": x_hat, **_yuv_metrics(frame, x_hat, yuv, write_to)}


@torch.no_grad()
def eval_gop(imodel, stem, frames, gop=12, all_intra=False, with_msssim=True, yuv=False, write_to=None, order="raster"):
    """frames: iterable of [3,h,w] images of ONE sequence, in display order (the script's f001.png, f002.png, ...).  Frame k
    (1-based) with k % gop == 1 is an I frame, every other one a P frame conditioned on the previous frame's decoded latents
    (stem/evalSTEM.py:186-209; gop = 12 for UVG, 10 for the HEVC classes).  Returns the per-frame dictionaries of the two
    inference functions (plus "type") and the sequence averages the script logs (:217-224).  with_msssim=False leaves the host-side
    MS-SSIM out (a reporting metric next to the codec path, ~0.3 s per 1080p frame on the host); with_msssim="device" takes "ms-ssim"
    and "psnr" of every frame from the HIP kernel instead (`_metrics`).  yuv=True adds "psnr_y", "psnr_u", "psnr_v", "psnr_yuv" to every
    frame (against the planes a data.YUVSequence frame carries, else against the frame quantised at 8 bits) and their averages
    "psnr_y_ave" ... "psnr_yuv_ave" to the result; write_to (a path or a binary file object) gets every decoded frame appended as raw
    planar 4:2:0 at the source's bit depth.  order="wavefront": every frame's y string in wavefront symbol order (codec.wave_order), the
    same reconstructions."""
    extra = {} if not yuv and write_to is None else {"yuv": yuv, "write_to": write_to}      # nothing new is passed through by default
    extra.update(_order_kw(order))
    per_frame, y_cond = [], None
    for index, x in enumerate(frames, start=1):
        if all_intra or index % gop == 1 or y_cond is None:
            out = inference_iframe(imodel, x, with_msssim, **extra)
            out["type"] = "I"
        else:
            out = inference_pframe(imodel, stem, x, y_cond, with_msssim, **extra)
            out["type"] = "P"
        y_cond = out["y_conditioned"]
        per_frame.append(out)
    n = max(1, len(per_frame))
    ms = [f["ms-ssim"] for f in per_frame if f["ms-ssim"] is not None]
    res = {"frames": per_frame, "psnr_ave": sum(f["psnr"] for f in per_frame) / n, "bpp_ave": sum(f["bpp"] for f in per_frame) / n,
           "msssim_ave": (sum(ms) / len(ms)) if ms else None,
           "estimate_bpp_ave": sum(f["estimate_bpp"] for f in per_frame) / n}
    if yuv:
        for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv"):
            res[k + "_ave"] = sum(f[k] for f in per_frame) / n
    return res


def gop_schedule(n_frames, gop, concurrent_gops, all_intra=False):
    """The order in which `eval_sequence` codes a sequence of `n_frames` frames (pure: no device).  A GOP is an I frame and the P frames
    that follow it, an independent chain; GOP boundaries are `eval_gop`'s (frame k, 1-based, with k % gop == 1 is an I frame, and so is the
    first frame; all_intra: every frame).  Up to `concurrent_gops` consecutive GOPs form a group whose chains advance together: step s of
    a group holds the s-th frame of each of its GOPs, a chain drops out when its GOP ends (the last GOP may be short, the last group
    small).  -> the list of steps, each a list of (frame index, 0-based, "I" | "P", chain = the GOP's number in the sequence)."""
    if gop < 1 or concurrent_gops < 1:
        raise ValueError(f"gop and concurrent_gops are at least 1, got {gop} and {concurrent_gops}")
    starts = [i for i in range(n_frames) if all_intra or i == 0 or (i + 1) % gop == 1]
    gops = [range(a, b) for a, b in zip(starts, starts[1:] + [n_frames])]
    steps = []
    for g0 in range(0, len(gops), concurrent_gops):
        group = list(enumerate(gops[g0:g0 + concurrent_gops], start=g0))
        for s in range(max(len(r) for _, r in group)):
            steps.append([(r[s], "I" if s == 0 else "P", chain) for chain, r in group if s < len(r)])
    return steps


class _InOrder:
    """`write_to` of eval_sequence: frames finish chain by chain, the file wants display order.  Every frame's planes arrive as bytes
    (already on the host) and wait until all earlier frames have been written."""

    def __init__(self, sink):
        self.sink, self.next, self.held = sink, 0, {}

    def put(self, index, data):
        self.held[index] = data
        while self.next in self.held:
            data = self.held.pop(self.next)
            if isinstance(self.sink, (str, os.PathLike)):
                with open(self.sink, "ab") as f:
                    f.write(data)
            else:
                self.sink.write(data)
            self.next += 1


@torch.no_grad()
def eval_sequence(imodel, stem, frames, gop=12, concurrent_gops=8, all_intra=False, with_msssim=True, yuv=False, write_to=None, order="raster"):
    """`eval_gop` with the sequence's GOPs coded side by side (`gop_schedule`): every GOP is an independent chain, and the raster-order
    coding loops -- launch- and latency-bound for one image -- advance up to `concurrent_gops` chains together (codec.iframe_*_each,
    codec.stem_*_each: one batched encoder queue, the concurrent / lockstep decoders).  Every transform still runs per chain at batch 1,
    so each frame's strings, latents and reconstruction are the bits `eval_gop` produces for it and decode on their own.
    frames: a sequence (indexable, with a length) or an iterable of [3,h,w] images of one size, in display order.  Returns what `eval_gop`
    returns: "frames" in display order, each with `eval_gop`'s keys and values, and the same averages.  Only the timing differs:
    "encoding_time" / "decoding_time" are the wall time of the frame's step divided by the number of chains in it, which the new key
    "concurrent" holds.  write_to receives the frames in display order.  concurrent_gops=1: one chain per step.  order: as in `eval_gop`."""
    from . import codec
    okw = _order_kw(order)
    if not (hasattr(frames, "__getitem__") and hasattr(frames, "__len__")):
        frames = list(frames)
    writer = _InOrder(write_to) if write_to is not None else None
    per_frame = [None] * len(frames)
    y_cond = {}                                                  # chain -> the decoded latents of its previous frame
    for step in gop_schedule(len(frames), gop, concurrent_gops, all_intra):
        srcs = [frames[i] for i, _, _ in step]
        xs = [f.unsqueeze(0) for f in srcs]
        padded = [bitstream.pad(x, 64) for x in xs]
        ipos = [k for k, (_, kind, _) in enumerate(step) if kind == "I"]
        ppos = [k for k, (_, kind, _) in enumerate(step) if kind == "P"]
        enc, fwd, dec, y_hat, x_hat = ([None] * len(step) for _ in range(5))
        _sync(xs[0])
        start = time.time()
        if ipos:
            for k, e in zip(ipos, codec.iframe_compress_each(imodel, [padded[k] for k in ipos], **okw)):
                enc[k] = e
                fwd[k] = imodel(padded[k])
        if ppos:
            conds = [y_cond[step[k][2]] for k in ppos]
            y_curs = [imodel.getY(padded[k])[0] for k in ppos]
            for k, y_cur, c in zip(ppos, y_curs, conds):
                fwd[k] = stem(y_cur, c)
            for k, e in zip(ppos, codec.stem_compress_each(stem, y_curs, conds, **okw)):
                enc[k] = e
        _sync(xs[0])
        enc_time = (time.time() - start) / len(step)
        start = time.time()
        if ipos:
            for k, d in zip(ipos, codec.iframe_decompress_each(imodel, [enc[k]["strings"] for k in ipos], [enc[k]["shape"] for k in ipos], **okw)):
                dec[k], y_hat[k], x_hat[k] = d, d["y_hat"], d["x_hat"]
        if ppos:
            outs = codec.stem_decompress_each(stem, [enc[k]["strings"] for k in ppos], [enc[k]["shape"] for k in ppos], conds, **okw)
            for k, y in zip(ppos, outs):
                dec[k] = {"y_hat": y} if stem.DECOMPRESS_RETURNS_DICT else y
                y_hat[k] = y
                x_hat[k] = imodel.getX(y)
        _sync(xs[0])
        dec_time = (time.time() - start) / len(step)
        for k, (index, kind, chain) in enumerate(step):
            x = xs[k]
            h, w = x.size(2), x.size(3)
            xh = bitstream.crop(x_hat[k], (h, w))
            num_pixels = x.size(0) * h * w
            bpp, est = _bpp_terms(enc[k], fwd[k], num_pixels)
            quality = _metrics(x, xh, with_msssim)
            sink = io.BytesIO() if writer is not None else None
            out = {"y_conditioned": y_hat[k], "psnr": quality[0], "ms-ssim": quality[1], "bpp": bpp, "estimate_bpp": sum(est.values()),
                   "estimate_y_bpp": est.get("y"), "estimate_z_bpp": est.get("z"), "y_bpp": len(enc[k]["strings"][0][0]) * 8.0 / num_pixels,
                   "z_bpp": len(enc[k]["strings"][1][0]) * 8.0 / num_pixels, "encoding_time": enc_time, "decoding_time": dec_time}
            if kind == "I":
                out["out_forward"] = fwd[k]
            else:
                out["entropy_params"] = dec[k].get("entropy_params") if isinstance(dec[k], dict) else None
            out.update({"strings": enc[k]["strings"], "shape": tuple(enc[k]["shape"]), "x_hat": xh, **_yuv_metrics(srcs[k], xh, yuv, sink),
                        "type": kind, "concurrent": len(step)})
            if writer is not None:
                writer.put(index, sink.getvalue())
            per_frame[index] = out
        y_cond = {chain: y_hat[k] for k, (_, _, chain) in enumerate(step)}      # a chain that left the step has ended
    n = max(1, len(per_frame))
    ms = [f["ms-ssim"] for f in per_frame if f["ms-ssim"] is not None]
    res = {"frames": per_frame, "psnr_ave": sum(f["psnr"] for f in per_frame) / n, "bpp_ave": sum(f["bpp"] for f in per_frame) / n,
           "msssim_ave": (sum(ms) / len(ms)) if ms else None,
           "estimate_bpp_ave": sum(f["estimate_bpp"] for f in per_frame) / n}
    if yuv:
        for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv"):
            res[k + "_ave"] = sum(f[k] for f in per_frame) / n
    return res
