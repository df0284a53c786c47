"""The evaluation loop of stem/evalSTEM.py (BASELINE configs[3]) as package functions.

    inference_iframe(imodel, x)                    stem/evalSTEM.py:34-89   (inferenceI_DVR)
    inference_pframe(imodel, stem, x, y_cond)      stem/evalSTEM.py:92-153  (inferenceP_DVR)
    eval_image(model, x) / eval_image_estimate     compressai/utils/eval_model/__main__.py:73-135 (inference, inference_entropy_estimation):
                                                   one image through an I-frame model of the zoo, outside any sequence
    eval_gop(imodel, stem, frames, gop=12)         the frame loop of evalDataset, stem/evalSTEM.py:180-216: frame index % GOP == 1
                                                   is an I frame coded by the image model's own compress / decompress, every other
                                                   frame a P frame conditioned on the previous frame's DECODED latents

    eval_sequence(imodel, stem, frames, ...)       `eval_gop` with the sequence's GOPs coded side by side (`gop_schedule`)

What these and the pixel-domain functions below share is stated once: `_code_image` (pad, timed encode, timed decode, crop of one still
image), `_frame_record` (a frame's dictionary; "z_bpp" is None for a model with one string) and `_sequence_averages`.
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

The pixel-domain models (models/stem_roi.py: stem_baseline, stem_baselinev2, stem_roi, stem_roi_wo_gsc, stem_roi_i) have the loop of
stem_roi/eval_stem_roi.py and stem_roi/eval_stem_baseline.py:

    quality_map(kind, h, w, level)                 the test-time maps of STEMTestDataset_Qmap, eval_stem_roi.py:77-93
    inference_pixel_i(model_i, x, qmap)            eval_stem_roi.py:112-166 / eval_stem_baseline.py:83-132  (inference_i)
    inference_pixel_p(model_p, x, x_cond, qmap)    eval_stem_roi.py:169-227 / eval_stem_baseline.py:134-187 (inference_p)
    eval_gop_pixel(model_i, model_p, frames, ...)  the frame loops, eval_stem_roi.py:230-354: a P frame is conditioned on the previous
                                                   frame's cropped reconstruction
    eval_levels(model_i, model_p, frames, levels)  the sweep over uniform levels of eval_rc, eval_stem_roi.py:368-375

These are pinned by tests/golden/pixel_eval_roi.npz and pixel_eval_baseline.npz (tests/golden/make_golden_pixel_eval.py runs the two
scripts' own functions) through
tests/test_hip_pixel_eval.py.

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


def _code_image(model, x, extra_ins=(), dec_ins=(), forward=True, **okw):
    """One still image x [1,3,h,w] through a model: centred zero pad to multiples of 64; model.compress(x_padded, *extra_ins) and, with
    forward=True, model(x_padded, *extra_ins) (the rate estimate) timed together as encoding; model.decompress(strings, shape, *dec_ins)
    timed as decoding; crop.  extra_ins / dec_ins arrive padded; okw goes to compress and decompress.
    -> (out_enc, out_forward or None, out_dec, the cropped x_hat, (encoding time, decoding time))"""
    ins = [bitstream.pad(x, 64), *extra_ins]
    _sync(x)
    start = time.time()
    out_enc = model.compress(*ins, **okw)
    out_forward = model(*ins) if forward else None
    _sync(x)
    enc_time = time.time() - start
    start = time.time()
    out_dec = model.decompress(out_enc["strings"], out_enc["shape"], *dec_ins, **okw)
    _sync(x)
    dec_time = time.time() - start
    return out_enc, out_forward, out_dec, bitstream.crop(out_dec["x_hat"], x.shape[-2:]), (enc_time, dec_time)


def _frame_record(x, x_hat, out_enc, out_forward, times, with_msssim, /, **extras):
    """One frame's dictionary, the keys every inference function shares: x, x_hat [1,3,h,w] the frame and its cropped reconstruction,
    out_enc what compress returned, out_forward what forward returned (the rate estimates), times = (encoding, decoding).  "z_bpp" is
    None for a model with one string (no hyper-prior).  extras: the caller's own keys, passed through."""
    num_pixels = x.size(0) * x.size(2) * x.size(3)
    strings = out_enc["strings"]
    bpp, est = _bpp_terms(out_enc, out_forward, num_pixels)
    quality = _metrics(x, x_hat, with_msssim)
    return {"psnr": quality[0], "ms-ssim": quality[1], "bpp": bpp, "estimate_bpp": sum(est.values()),
            "estimate_y_bpp": est.get("y"), "estimate_z_bpp": est.get("z"), "y_bpp": len(strings[0][0]) * 8.0 / num_pixels,
            "z_bpp": len(strings[1][0]) * 8.0 / num_pixels if len(strings) > 1 else None,
            "encoding_time": times[0], "decoding_time": times[1], "strings": strings, "shape": tuple(out_enc["shape"]), "x_hat": x_hat, **extras}


_YUV_KEYS = ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv")


def _sequence_averages(per_frame, also=(), psnr_roi=False):
    """A sequence's result: "frames" and the averages the scripts log (stem/evalSTEM.py:217-224, eval_stem_roi.py:343-354) --
    "psnr_ave", "bpp_ave", "estimate_bpp_ave" over every frame, "msssim_ave" over the frames that have an MS-SSIM (None without any).
    also: further per-frame keys averaged over every frame (`_YUV_KEYS`, "bits"); psnr_roi: "psnr_roi_ave", the mean over the frames
    with a finite "psnr_roi", None without any."""
    n = max(1, len(per_frame))
    ms = [f["ms-ssim"] for f in per_frame if f["ms-ssim"] is not None]
    res = {"frames": per_frame, "psnr_ave": sum(f["psnr"] for f in per_frame) / n, "bpp_ave": sum(f["bpp"] for f in per_frame) / n,
           "msssim_ave": (sum(ms) / len(ms)) if ms else None,
           "estimate_bpp_ave": sum(f["estimate_bpp"] for f in per_frame) / n}
    for k in also:
        res[k + "_ave"] = sum(f[k] for f in per_frame) / n
    if psnr_roi:
        roi = [f["psnr_roi"] for f in per_frame if f.get("psnr_roi") is not None and math.isfinite(f["psnr_roi"])]
        res["psnr_roi_ave"] = (sum(roi) / len(roi)) if roi else None
    return res


@torch.no_grad()
def inference_iframe(model, x, with_msssim=True, yuv=False, write_to=None, order="raster"):
    """x: one image [3,h,w] in [0,1].  Pad to multiples of 64 (centred), compress + forward (the rate estimate), decompress, crop.
    `y_conditioned` is the DECODED latent of the padded image: what the next P frame is conditioned on.  yuv, write_to: `_yuv_metrics`;
    order: the symbol order of the y string ("raster" | "wavefront")."""
    okw = _order_kw(order)
    frame, x = x, x.unsqueeze(0)
    out_enc, out_forward, out_dec, x_hat, times = _code_image(model, x, **okw)
    return _frame_record(x, x_hat, out_enc, out_forward, times, with_msssim, y_conditioned=out_dec["y_hat"], out_forward=out_forward,
                         **_yuv_metrics(frame, x_hat, yuv, write_to))


@torch.no_grad()
def eval_image(model, x, with_msssim="device"):
    """compressai/utils/eval_model/__main__.py:73-113 (`inference`) for any of the six zoo models.  x: one image [3,h,w] in [0,1]:
    centred zero pad to multiples of 64, compress, decompress, crop -> {"psnr", "ms-ssim", "bpp", "encoding_time",
    "decoding_time"}, bpp from the lengths of the strings.  "ms-ssim" comes from the device metric (`with_msssim`: see `_metrics`;
    None for images without a fifth scale, where the reference's package raises)."""
    x = x.unsqueeze(0)
    out_enc, _, _, x_hat, times = _code_image(model, x, forward=False)
    quality = _metrics(x, x_hat, with_msssim)
    return {"psnr": quality[0], "ms-ssim": quality[1], "bpp": sum(len(s[0]) for s in out_enc["strings"]) * 8.0 / (x.size(0) * x.size(2) * x.size(3)),
            "encoding_time": times[0], "decoding_time": times[1]}


@torch.no_grad()
def eval_image_estimate(model, x):
    """eval_model/__main__.py:116-135 (`inference_entropy_estimation`): the forward pass on the image as it is (no padding, as
    there: sides the model's strides do not divide raise a shape error) -> {"psnr", "bpp", "encoding_time", "decoding_time"}, bpp
    the rate estimate -sum(log2 likelihoods) / pixels."""
    x = x.unsqueeze(0)
    _sync(x)
    start = time.time()
    out_net = model(x)
    _sync(x)
    elapsed = time.time() - start
    num_pixels = x.size(0) * x.size(2) * x.size(3)
    x_hat = out_net["x_hat"]
    if tuple(x_hat.shape) != tuple(x.shape):
        raise ValueError(f"eval_image_estimate: the model returns {tuple(x_hat.shape[-2:])} for an image of {tuple(x.shape[-2:])}: "
                         f"pad it to multiples of the model's downsampling factor")
    bpp = sum(_bpp_terms({"strings": []}, out_net, num_pixels)[1].values())
    return {"psnr": psnr(x, x_hat), "bpp": bpp, "encoding_time": elapsed / 2.0, "decoding_time": elapsed / 2.0}


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
    return _frame_record(x, x_hat, out_enc, out_forward, (enc_time, dec_time), with_msssim, y_conditioned=y_hat,
                         entropy_params=out_dec.get("entropy_params") if isinstance(out_dec, dict) else None,
                         **_yuv_metrics(frame, x_hat, yuv, write_to))


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
    return _sequence_averages(per_frame, _YUV_KEYS if yuv else ())


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
            xh = bitstream.crop(x_hat[k], xs[k].shape[-2:])
            sink = io.BytesIO() if writer is not None else None
            own = {"out_forward": fwd[k]} if kind == "I" else {"entropy_params": dec[k].get("entropy_params") if isinstance(dec[k], dict) else None}
            per_frame[index] = _frame_record(xs[k], xh, enc[k], fwd[k], (enc_time, dec_time), with_msssim, y_conditioned=y_hat[k], **own,
                                             **_yuv_metrics(srcs[k], xh, yuv, sink), type=kind, concurrent=len(step))
            if writer is not None:
                writer.put(index, sink.getvalue())
        y_cond = {chain: y_hat[k] for k, (_, _, chain) in enumerate(step)}      # a chain that left the step has ended
    return _sequence_averages(per_frame, _YUV_KEYS if yuv else ())


# ----------------------------------------------------------------------------- pixel-domain models (stem_roi/eval_stem_*.py)
def quality_map(kind, h, w, level=0, level_range=(0, 100)):
    """A test-time quality map [1,1,h,w] float32 (host tensor), values in [0, 1] (eval_stem_roi.py:77-93):
        "uniform"     level / level_range[1] everywhere
        "horizontal"  np.linspace(0, 1, w) in every row
        "vertical"    np.linspace(0, 1, h) in every column
    computed in float64 with numpy, then cast, as the script does.  The script's vertical branch tiles linspace(0, 1, h) into a
    (1, h * w) array, which no model accepts; what is built here is its evident intent, the transpose of the horizontal map.
    A tensor [h,w] / [1,h,w] / [1,1,h,w] (an ROI mask) is returned as [1,1,h,w] float32 with its values untouched."""
    import numpy as np
    if torch.is_tensor(kind):
        if tuple(kind.shape[-2:]) != (h, w) or kind.dim() not in (2, 3, 4) or any(d != 1 for d in kind.shape[:-2]):
            raise ValueError(f"a quality map for a {h} x {w} frame is [h,w], [1,h,w] or [1,1,h,w], got {tuple(kind.shape)}")
        return kind.reshape(1, 1, h, w).float()
    if kind == "uniform":
        q = np.full((h, w), float(level) / float(level_range[1]), dtype=np.float64)
    elif kind == "horizontal":
        q = np.tile(np.linspace(0, 1, w), (h, 1))
    elif kind == "vertical":
        q = np.tile(np.linspace(0, 1, h)[:, None], (1, w))
    else:
        raise ValueError(f'quality_map kind is "uniform", "horizontal", "vertical" or a tensor, got {kind!r}')
    return torch.from_numpy(q.astype(np.float32)).reshape(1, 1, h, w)


def _takes_qmap(model):
    return bool(getattr(model, "QMAP", False))


def psnr_roi(x, x_hat, weight):
    """-10 log10(sum w (x - x_hat)^2 / (3 sum w)) of one frame [1,3,h,w] under the weight map [1,1,h,w]: the weighted squared error by
    the HIP reduction (functional.weighted_sqerr_sum, accumulated in float64), sum w in float64.  None when sum w == 0."""
    from . import functional
    if tuple(weight.shape) != (x.shape[0], 1, x.shape[2], x.shape[3]):
        raise ValueError(f"roi_weight for a frame {tuple(x.shape)} is [B,1,h,w], got {tuple(weight.shape)}")
    if not (x.is_cuda and x_hat.is_cuda and weight.is_cuda):
        raise RuntimeError("psnr_roi runs the HIP reduction: the frame, its reconstruction and the weight map must be device tensors")
    total = float(weight.double().sum())
    if total == 0:
        return None
    sse = float(functional.weighted_sqerr_sum(x_hat.float().contiguous(), x.float().contiguous(), weight.contiguous()))
    return -10 * math.log10(sse / (x.shape[1] * total)) if sse > 0 else float("inf")


def _pixel_frame(model, x, x_conditioned, qmap, with_msssim, roi_weight):
    """inference_i / inference_p of the two scripts: one body, the condition and the map passed where the model takes them"""
    x = x.unsqueeze(0) if x.dim() == 3 else x
    h, w = x.size(2), x.size(3)
    if qmap is not None:
        qmap = quality_map(qmap, h, w).to(x.device)
    if roi_weight is None:
        roi_weight = qmap
    elif roi_weight is False:
        roi_weight = None
    else:
        roi_weight = quality_map(roi_weight, h, w).to(x.device)
    cond = []
    if x_conditioned is not None:
        cond = [bitstream.pad(x_conditioned.unsqueeze(0) if x_conditioned.dim() == 3 else x_conditioned, 64)]
    ins = list(cond)
    if _takes_qmap(model):
        if qmap is None:
            raise ValueError(f"{type(model).__name__} takes a quality map")
        ins.append(bitstream.pad(qmap, 64))
    out_enc, out_forward, _, x_hat, times = _code_image(model, x, ins, cond)
    out = _frame_record(x, x_hat, out_enc, out_forward, times, with_msssim, bits=sum(len(s[0]) for s in out_enc["strings"]) * 8.0)
    if roi_weight is not None:
        out["psnr_roi"] = psnr_roi(x, x_hat, roi_weight)
    return out


@torch.no_grad()
def inference_pixel_i(model_i, x, qmap=None, with_msssim=True, roi_weight=None):
    """x: one image [3,h,w] in [0,1]; qmap: what `quality_map` passes through, or None.  The frame and the map are zero-padded to
    multiples of 64 (centred), then compress + forward (the rate estimate), decompress, crop (eval_stem_roi.py:112-166,
    eval_stem_baseline.py:83-132).  The map goes to the models that take one (stem_roi_i); every I-frame model whose compress /
    decompress return "strings", "shape" and "x_hat" is accepted (MeanScaleHyperprior, mbt2018).  Keys as `inference_iframe`, plus
    "bits"; with a weight map -- roi_weight, by default the quality map, False for none -- also "psnr_roi" (`psnr_roi`)."""
    return _pixel_frame(model_i, x, None, qmap, with_msssim, roi_weight)


@torch.no_grad()
def inference_pixel_p(model_p, x, x_conditioned, qmap=None, with_msssim=True, roi_weight=None):
    """`inference_pixel_i` for a P-frame model: x_conditioned [3,h,w] or [1,3,h,w], the previous frame's reconstruction at the
    frame's own size, is zero-padded like the frame (eval_stem_roi.py:169-227, eval_stem_baseline.py:134-187)."""
    return _pixel_frame(model_p, x, x_conditioned, qmap, with_msssim, roi_weight)


def _per_frame_maps(qmaps):
    """the four forms of eval_gop_pixel's `qmaps` -> a function (index, h, w) -> map or None"""
    if qmaps is None:
        return lambda index, h, w: None
    if callable(qmaps):
        return qmaps
    if torch.is_tensor(qmaps):
        return lambda index, h, w: qmaps
    it = iter(qmaps)

    def following(index, h, w):
        try:
            return next(it)
        except StopIteration:
            raise ValueError(f"qmaps ran out at frame {index}: an iterable of maps is parallel to the frames") from None

    return following


@torch.no_grad()
def eval_gop_pixel(model_i, model_p, frames, qmaps=None, gop=12, all_intra=False, with_msssim=True, roi_weight=None):
    """The frame loop of the two scripts (eval_stem_roi.py:230-354) over ONE sequence.  frames: iterable of [3,h,w] images in display
    order.  Frame k (1-based) with k % gop == 1 is an I frame (model_i), every other one a P frame (model_p) conditioned on the previous
    frame's CROPPED x_hat, which is zero-padded again: the border of the condition is zero, not the decoder's padded reconstruction
    (:237-242).  With gop == 1 that rule never fires after the first frame (k % 1 == 0): the sequence is coded I P P P ..., as `eval_gop`
    does, where the script's loader (eval_stem_roi.py:96, index % gop == 0) would make every frame intra -- ask for that with all_intra.
    qmaps: None; one map for every frame; an iterable of maps parallel to `frames`; or a callable (index, h, w) -> map
    with the 0-based frame index.  A map is anything `quality_map` passes through.  roi_weight: as in `inference_pixel_i`, one for every
    frame.  -> {"frames": the per-frame dictionaries plus "type", "psnr_ave", "msssim_ave", "bpp_ave", "bits_ave", "estimate_bpp_ave",
    "psnr_roi_ave"}; the last is the mean over the frames that have a finite "psnr_roi", None without any."""
    map_of = _per_frame_maps(qmaps)
    per_frame, x_cond = [], None
    for index, x in enumerate(frames):
        q = map_of(index, x.size(-2), x.size(-1))
        if all_intra or (index + 1) % gop == 1 or x_cond is None:
            out = inference_pixel_i(model_i, x, q, with_msssim, roi_weight)
            out["type"] = "I"
        else:
            out = inference_pixel_p(model_p, x, x_cond, q, with_msssim, roi_weight)
            out["type"] = "P"
        x_cond = out["x_hat"]
        per_frame.append(out)
    return _sequence_averages(per_frame, ("bits",), psnr_roi=True)


def eval_levels(model_i, model_p, frames, levels=(0.30, 0.45, 0.55, 0.70), gop=12, level_range=(0, 1), **kwargs):
    """The rate sweep of eval_rc / _eval_stem_roi_seq_rc (eval_stem_roi.py:307-375): one `eval_gop_pixel` per level with the uniform
    map level / level_range[1] on every frame.  frames must be re-iterable (a list, a data.YUVSequence): every level reads it again.
    kwargs: `eval_gop_pixel`'s (all_intra, with_msssim, roi_weight).  -> {level: result}."""
    if iter(frames) is frames:
        raise ValueError("eval_levels reads the frames once per level: pass a list or another re-iterable sequence, not an iterator")
    return {level: eval_gop_pixel(model_i, model_p, frames, qmaps=lambda index, h, w, level=level: quality_map("uniform", h, w, level, level_range),
                                  gop=gop, **kwargs) for level in levels}
