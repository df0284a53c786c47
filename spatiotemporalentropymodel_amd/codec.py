"""compress() / decompress() of the STEM models: transforms and per-position probability model on the GPU,
rANS on the host (north_star), bitstreams interchangeable with the reference's
(compressai/models/spatiotemporalpriors.py:86-111, 197-225, 871-1054).

Models without a spatial prior are coded in one shot.  Models with the masked-convolution prior are coded
in raster order: position (h, w) needs the *decoded* values to its left and above, so each position is a
chain of four matrix-vector kernels (csrc/ar.hip) on one pixel; the encoder queues the whole frame
asynchronously (wavefront-parallel, t = w + 3h) and calls the host coder once; the decoder's raster-order loop runs
inside the library (stem_ar_decode_image): per position four launches (the first also writes back the previous pixel,
the last also emits the CDF indexes), one stream synchronisation and one call of the host rANS decoder -- injected as a
C function pointer -- through a pinned mailbox.  (A cooperative single-launch variant was measured slower on ROCm 7.2:
0.74 s vs 0.44 s per 1080p frame.)  By default one persistent kernel per image instead (csrc/ar_persistent.hip);
`decode_route` names every form of the loop and says which one runs.  All forms are bit-identical.  A batch is encoded in lockstep
(stem_ar_encode_batch: one queue of wavefront steps for all images, one copy, the host coder per image on a thread pool), and the
`*_each` entry points code several independent chains -- the GOPs evaluation.eval_sequence walks side by side -- with every transform
at batch 1 and only the coding loops batched.

`order="wavefront"` (every compress / decompress entry point; default "raster", the reference's) codes the same symbols in the order of
the encoder's wavefront steps (`wave_order`; include/stem_ar_batch.h states it): the decoder then advances a step of positions per host
round trip -- W + 3(H-1) of them instead of H * W -- with the encoder's own launches (stem_ar_decode_wave_batch).  Every quantised value
is that of the raster route; the y string is this project's own format, which the reference's decoder cannot read.
"""
from __future__ import annotations

import ctypes as C
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from . import config as _config
from . import functional as F
from .entropy_models import BufferedRansEncoder, RansDecoder
from .weights import closed_form_input

_K = 5      # context kernel size
_P = 2      # its padding


ORDERS = ("raster", "wavefront")


def _check_order(order, model=None):
    """`order` names a symbol order, and the model has a raster loop to reorder (asked before any device work)"""
    if order not in ORDERS:
        raise ValueError(f"order is one of {ORDERS}, got {order!r}")
    if order == "wavefront" and model is not None and not model.HAS_SPM:
        raise ValueError(f'order="wavefront": {type(model).__name__} has no spatial prior -- its latents are coded in one shot, there is no '
                         "raster-order loop whose symbols could be reordered")


def wave_order(H, W):
    """The wavefront symbol order of an H x W latent (pure: numpy only).  Steps run t = 0 .. W + 3(H-1) - 1; within a step rows run
    h = h0(t) .. h0(t) + np(t) - 1 ascending with w = t - 3h (h0, np: wave_range of csrc/ar_canon.h); within a position the channels run
    0 .. M-1.  -> (the raster indices h * W + w in wavefront order, int64 [H*W]; the step sizes np(t), int64 [W + 3(H-1)])"""
    if H < 1 or W < 1:
        raise ValueError(f"wave_order: a latent has at least one position, got {H} x {W}")
    order, sizes = [], []
    for t in range(W + 3 * (H - 1)):
        lo = t - (W - 1)
        h0 = (lo + 2) // 3 if lo > 0 else 0
        h1 = min(t // 3, H - 1)
        sizes.append(max(0, h1 - h0 + 1))
        order.extend(h * W + (t - 3 * h) for h in range(h0, h1 + 1))
    return np.asarray(order, dtype=np.int64), np.asarray(sizes, dtype=np.int64)


def _chain(layers, x):
    """the three convolutions of a hyper / prior / entropy-parameter stack, LeakyReLU between them"""
    return layers[2].fwd(layers[1].fwd(layers[0].fwd(x, F.ACT_LRELU), F.ACT_LRELU))


def _check_latent_size(latent, prior, what):
    if tuple(prior.shape[-2:]) != tuple(latent.shape[-2:]):
        raise ValueError(f"latent size {tuple(latent.shape[-2:])} does not survive the two stride-2 hyper stages (hyper-prior is "
                         f"{tuple(prior.shape[-2:])}): pad {what} to multiples of 64 pixels, as stem/evalSTEM.py:95-108 does")


def _hyper(model, y_cur, y_cond, strings_z=None, shape=None):
    """z path shared by compress / decompress: returns (z_strings, z_shape, hp, tp) with hp/tp dense NHWC tensors (tp may be None)."""
    eng = model.engine()
    eb = model.entropy_bottleneck
    yd = F.to_nhwc(y_cond.detach())
    if strings_z is None:
        yc = F.to_nhwc(y_cur.detach())
        B, Cin, H, W = yc.shape
        he_in = F.empty_nhwc(B, 2 * Cin, H, W, yc.device)
        F.copy_channels(yc, he_in[:, :Cin])
        F.copy_channels(yd, he_in[:, Cin:])
        z = _chain(eng.HE, he_in)
        strings_z = eb.compress(z)
        shape = z.shape[-2:]
    z_hat = eb.decompress(strings_z, shape).to(yd.device).float()
    hp = _chain(eng.HD, F.to_nhwc(z_hat))
    _check_latent_size(yd, hp, "frames")
    tp = _chain(eng.TPM, yd) if eng.has_tpm else None
    return strings_z, shape, hp, tp


def _one_shot(model, hp, tp):
    """no spatial prior: EPM on the concatenated priors (dense NHWC) -> gp = scales | means, returned as the two channel slices (scales, means)"""
    priors = [p for p in (tp, hp) if p is not None]
    B, P, H, W = hp.shape
    epm_in = F.empty_nhwc(B, P * len(priors), H, W, hp.device)
    for i, p in enumerate(priors):
        F.copy_channels(p, epm_in[:, i * P:(i + 1) * P])
    gp = _chain(model.engine().EPM, epm_in)
    return gp[:, :P // 2], gp[:, P // 2:]


class _ARContext:
    """Per-model device state of the raster-order loop: GEMV-layout weights and scratch vectors."""

    def __init__(self, model, device):
        m = model
        M = m.in_channels
        self.M = M
        w = m.context_prediction.weight.detach().contiguous()
        self.w_ctx = torch.empty((2 * M, 12 * M), device=device, dtype=torch.float32)
        F._chk(_lib.hip().stem_pack_ctx_gemv(w.data_ptr(), self.w_ctx.data_ptr(), 2 * M, M, F._stream()))
        self.b_ctx = m.context_prediction.bias.detach()
        # The coding kernels take hidden widths that are multiples of 4.  M * 10 // 3 and M * 8 // 3 are that for M = 96, 192, 320 but
        # not for the M = N = 128 (426, 341) or 64 of the cheng2020 models: their two hidden layers get zero rows (and the next
        # layer zero columns) up to the next multiple.  A padded unit is lrelu(0) = 0 and meets a zero weight: every real sum keeps
        # its terms and their order.  Widths that are multiples of 4 already are left as they are.
        n0, n1 = (-(-m.EPM[i].out_channels // 4) * 4 for i in (0, 2))

        def padded(t, *shape):
            t = t.detach().reshape(t.shape[0], -1) if t.dim() == 4 else t.detach()
            if tuple(t.shape) == shape:
                return t.contiguous()
            out = torch.zeros(shape, device=t.device, dtype=t.dtype)
            out[tuple(slice(0, s) for s in t.shape)] = t
            return out
        self.w0 = padded(m.EPM[0].weight, n0, m.EPM[0].in_channels)
        self.w1 = padded(m.EPM[2].weight, n1, n0)
        self.w2 = padded(m.EPM[4].weight, m.EPM[4].out_channels, n1)
        self.b0, self.b1, self.b2 = padded(m.EPM[0].bias, n0), padded(m.EPM[2].bias, n1), m.EPM[4].bias.detach()
        self.ctx = torch.empty(2 * M, device=device)
        self.h1 = torch.empty(self.w0.shape[0], device=device)
        self.h2 = torch.empty(self.w1.shape[0], device=device)
        self.gp = torch.empty(2 * M, device=device)
        self.table = m.gaussian_conditional.scale_table.to(device).float().contiguous()
        self.bound = m.gaussian_conditional._scale_bound
        self.has_tpm = m.HAS_TPM

    def net_args(self):
        """what every stem_ar_* image call begins with: the context product, then the three EPM products as weights, row length, bias (, rows)"""
        M = self.M
        return (self.w_ctx.data_ptr(), 12 * M, self.b_ctx.data_ptr(), self.w0.data_ptr(), self.w0.shape[1], self.b0.data_ptr(), self.w0.shape[0],
                self.w1.data_ptr(), self.w1.shape[1], self.b1.data_ptr(), self.w1.shape[0], self.w2.data_ptr(), self.w2.shape[1], self.b2.data_ptr())

    def table_args(self):
        """scale table, its length, the scale bound, the LeakyReLU slope: what follows the scratch pointers in those calls"""
        return self.table.data_ptr(), self.table.numel(), self.bound, F.LRELU_SLOPE

    def scratch_args(self):
        """one image's intermediate vectors: context output, the two hidden layers, scales | means"""
        return self.ctx.data_ptr(), self.h1.data_ptr(), self.h2.data_ptr(), self.gp.data_ptr()

    def encode_wavefront(self, buf, H, W, tp_b, hp_b, sym, idx):
        """All positions with equal t = w + 3h are independent under the 5x5 type-A mask: W + 3(H-1) batched steps
        (csrc/ar.hip) instead of H*W sequential ones; symbols / indexes are written in raster order."""
        lib, M, st = _lib.hip(), self.M, F._stream()
        P, Wp = 2 * M, W + 2 * _P
        npmax = min(H, (W + 2) // 3)
        n1, n2 = self.w0.shape[0], self.w1.shape[0]
        wctx, wh1, wh2, wgp = (torch.empty((npmax, n), device=buf.device) for n in (P, n1, n2, P))
        if not _config.runtime().ar_stepwise:
            # all W + 3(H-1) steps queued by one library call (no interpreter between the 5 launches of a step)
            F._chk(lib.stem_ar_encode_image(*self.net_args(), buf.data_ptr(), H, W, M, _P, tp_b, hp_b,
                                            wctx.data_ptr(), wh1.data_ptr(), wh2.data_ptr(), wgp.data_ptr(), *self.table_args(),
                                            sym.data_ptr(), idx.data_ptr(), st))
            return
        S = _lib.WaveSeg
        base = buf.data_ptr()
        row = Wp * M
        seg_ctx = (S * 3)(S(base, 5 * M, 0, row, M, 0), S(base + 4 * row, 5 * M, 5 * M, row, M, 0), S(base + 8 * row, 2 * M, 10 * M, row, M, 0))
        ctx_seg = S(wctx.data_ptr(), P, 0, 0, 0, P)
        if self.has_tpm:
            ctx_seg.woff = 2 * P
            seg_e0 = (S * 3)(S(tp_b, P, 0, W * P, P, 0), S(hp_b, P, P, W * P, P, 0), ctx_seg)
        else:
            ctx_seg.woff = P
            seg_e0 = (S * 3)(S(hp_b, P, 0, W * P, P, 0), ctx_seg, S(0, 0, 0, 0, 0, 0))
        seg_e1 = (S * 3)(S(wh1.data_ptr(), n1, 0, 0, 0, n1), S(0, 0, 0, 0, 0, 0), S(0, 0, 0, 0, 0, 0))
        seg_e2 = (S * 3)(S(wh2.data_ptr(), n2, 0, 0, 0, n2), S(0, 0, 0, 0, 0, 0), S(0, 0, 0, 0, 0, 0))
        a_ctx, a_e0, a_e1, a_e2 = (C.addressof(x) for x in (seg_ctx, seg_e0, seg_e1, seg_e2))
        for t in range(W + 3 * (H - 1)):
            F._chk(lib.stem_gemv3_wave(self.w_ctx.data_ptr(), 12 * M, self.b_ctx.data_ptr(), a_ctx, wctx.data_ptr(), P, P, 0, 0.0, t, H, W, st))
            F._chk(lib.stem_gemv3_wave(self.w0.data_ptr(), self.w0.shape[1], self.b0.data_ptr(), a_e0, wh1.data_ptr(), n1, n1,
                                       F.ACT_LRELU, F.LRELU_SLOPE, t, H, W, st))
            F._chk(lib.stem_gemv3_wave(self.w1.data_ptr(), self.w1.shape[1], self.b1.data_ptr(), a_e1, wh2.data_ptr(), n2, n2,
                                       F.ACT_LRELU, F.LRELU_SLOPE, t, H, W, st))
            F._chk(lib.stem_gemv3_wave(self.w2.data_ptr(), self.w2.shape[1], self.b2.data_ptr(), a_e2, wgp.data_ptr(), P, P, 0, 0.0, t, H, W, st))
            F._chk(lib.stem_ar_finish_encode_wave(wgp.data_ptr(), self.table.data_ptr(), self.table.numel(), self.bound,
                                                  buf.data_ptr(), sym.data_ptr(), idx.data_ptr(), M, t, H, W, Wp, _P, st))

    def encode_batch(self, buf, G, H, W, tp_b, hp_b, sym, idx):
        """G images in lockstep (csrc/ar.hip: stem_ar_encode_batch): the five launches of a wavefront step cover all G images, whose
        arithmetic -- and so every symbol and index -- is that of `encode_wavefront` image by image.  buf [G, H+4, W+4, M]; sym / idx
        [G, H*W, M]; tp_b / hp_b: where the first image's priors start."""
        M, P = self.M, 2 * self.M
        npmax = min(H, (W + 2) // 3)
        scratch = [torch.empty((G, npmax, n), device=buf.device) for n in (P, self.w0.shape[0], self.w1.shape[0], P)]
        F._chk(_lib.hip().stem_ar_encode_batch(*self.net_args(), buf.data_ptr(), G, H, W, M, _P, tp_b, hp_b, *[t.data_ptr() for t in scratch],
                                               *self.table_args(), sym.data_ptr(), idx.data_ptr(), F._stream()))

    def position_decode(self, buf, Wp, h, w, tp_pix, hp_pix, sym_prev, pix_prev, prev_is_left, idx_out):
        """The four products of position (h, w) as the decoder issues them (_Decode.stepwise): the first also writes back the previous
        position's y_hat (and uses it in place of the not-yet-visible left neighbour), the last one also emits the CDF indexes."""
        lib, M, st = _lib.hip(), self.M, F._stream()
        base = buf.data_ptr()
        r0 = base + 4 * ((h * Wp + w) * M)
        r1 = base + 4 * (((h + 1) * Wp + w) * M)
        r2 = base + 4 * (((h + 2) * Wp + w) * M)
        mean_prev = self.gp.data_ptr() + 4 * M
        F._chk(lib.stem_gemv3_decode(self.w_ctx.data_ptr(), 12 * M, self.b_ctx.data_ptr(), r0, 5 * M, 0, r1, 5 * M, 5 * M, r2, 2 * M, 10 * M,
                                     self.ctx.data_ptr(), 2 * M, 0, 0.0, sym_prev, mean_prev, pix_prev, M, int(bool(prev_is_left and sym_prev)),
                                     0, 0, 0.0, 0, st))
        P = 2 * M
        if self.has_tpm:
            segs = (tp_pix, P, 0, hp_pix, P, P, self.ctx.data_ptr(), P, 2 * P)
        else:
            segs = (hp_pix, P, 0, self.ctx.data_ptr(), P, P, 0, 0, 0)
        F._chk(lib.stem_gemv3(self.w0.data_ptr(), self.w0.shape[1], self.b0.data_ptr(), *segs, self.h1.data_ptr(),
                              self.w0.shape[0], F.ACT_LRELU, F.LRELU_SLOPE, st))
        F._chk(lib.stem_gemv3(self.w1.data_ptr(), self.w1.shape[1], self.b1.data_ptr(), self.h1.data_ptr(), self.w1.shape[1], 0,
                              0, 0, 0, 0, 0, 0, self.h2.data_ptr(), self.w1.shape[0], F.ACT_LRELU, F.LRELU_SLOPE, st))
        F._chk(lib.stem_gemv3_decode(self.w2.data_ptr(), self.w2.shape[1], self.b2.data_ptr(), self.h2.data_ptr(), self.w2.shape[1], 0,
                                     0, 0, 0, 0, 0, 0, self.gp.data_ptr(), self.w2.shape[0], 0, 0.0, 0, 0, 0, M, 0,
                                     self.table.data_ptr(), self.table.numel(), self.bound, idx_out, st))


def _padded(target_img, H, W, M, device):
    """[Hp, Wp, M] zero-padded NHWC copy of one image's latent (F.pad(..., (2,2,2,2)), :898)."""
    buf = torch.zeros((H + 2 * _P, W + 2 * _P, M), device=device, dtype=torch.float32)
    if target_img is not None:
        inner = buf[_P:_P + H, _P:_P + W].permute(2, 0, 1).unsqueeze(0)          # [1,M,H,W] view, pitch-strided rows
        inner.copy_(target_img)                                                   # one small strided copy per image
    return buf


def _unpad_into(out, b, buf, H, W):
    """the interior of image b's padded buffer -> out[b]"""
    out[b:b + 1].copy_(buf[_P:_P + H, _P:_P + W].permute(2, 0, 1).unsqueeze(0))


def _prior_addrs(tp, hp, b, H, W, M):
    """(tp_b, hp_b): where image b starts in the dense NHWC [B, 2M, H, W] priors; tp_b = 0 without a temporal prior"""
    off = 4 * (b * H * W * 2 * M)
    return (tp.data_ptr() + off if tp is not None else 0), hp.data_ptr() + off


def _decoder_on(string):
    dec = RansDecoder()
    dec.set_stream(string)
    return dec


def _result(y_strings, z_strings, zshape, order, y_hat=None):
    """what compress returns; "order" only where it is not the reference's and "y_hat" only where it was asked for, so default results
    are the dictionaries they were"""
    res = {"strings": [y_strings, z_strings], "shape": zshape}
    if order != "raster":
        res["order"] = order
    if y_hat is not None:
        res["y_hat"] = y_hat
    return res


def _decoded(model, rec, yd):
    """the encoder's reconstruction `rec` of the coded target as the latent `stem_decompress` returns: plus y_cond for the residual classes"""
    return F.add(rec, _dense(yd)) if model.RESIDUAL else rec


def stem_compress(model, y_cur, y_cond, order="raster", return_y_hat=False):
    """return_y_hat=True: the result gains "y_hat", the latent `stem_decompress` of these strings returns, taken from the encoder's own
    state (the coder's buffer, or the symbols still on the device for the one-shot models): no decoder runs"""
    _check_order(order, model)
    z_strings, zshape, hp, tp = _hyper(model, y_cur, y_cond)
    yc, yd = F.to_nhwc(y_cur.detach()), F.to_nhwc(y_cond.detach())
    target = F.sub(_dense(yc), _dense(yd)) if model.RESIDUAL else _dense(yc)
    rec = None
    if not model.HAS_SPM:
        scales, means = _one_shot(model, hp, tp)
        y_strings = model.gaussian_conditional.compress(target, None, means=means, scales=scales, return_y_hat=return_y_hat)
        if return_y_hat:
            y_strings, rec = y_strings
    elif return_y_hat:
        y_strings, rec = _encode_latents(model, target, hp, tp, order, want_y_hat=True)
    else:
        y_strings = _encode_latents(model, target, hp, tp, order)
    return _result(y_strings, z_strings, zshape, order, _decoded(model, rec, yd) if return_y_hat else None)


def _encode_latents(model, target, hp, tp, order="raster", want_y_hat=False):
    """the raster-order coding of `target` (dense NHWC [B, M, H, W]) given the hyper prior `hp` and the temporal prior `tp` (or
    None): spatiotemporalpriors.py:916-961 / priors.py:586-631 -> one string per image.  order="wavefront": the same symbols and
    indexes, handed to the host coder in the order of `wave_order`.  want_y_hat: -> (strings, the reconstruction the coding kernels left
    in their padded buffers, dense NHWC [B, M, H, W]) -- what `_decode_latents` of the strings gives, under either order."""
    _check_order(order)
    B, M, H, W = target.shape
    dev = target.device
    ar = _ARContext(model, dev)
    tables = model.gaussian_conditional.host_tables()
    si = torch.empty((2, B, H * W, M), device=dev, dtype=torch.int32)             # symbols | indexes of the batch, raster order per image
    y_hat = F.empty_nhwc(B, M, H, W, dev) if want_y_hat else None
    if B > 1 and not _config.runtime().ar_stepwise:
        # one queue of wavefront steps for the whole batch
        buf = torch.zeros((B, H + 2 * _P, W + 2 * _P, M), device=dev, dtype=torch.float32)
        buf[:, _P:_P + H, _P:_P + W].permute(0, 3, 1, 2).copy_(target)
        ar.encode_batch(buf, B, H, W, *_prior_addrs(tp, hp, 0, H, W, M), si[0], si[1])
        if want_y_hat:
            y_hat.copy_(buf[:, _P:_P + H, _P:_P + W].permute(0, 3, 1, 2))
    else:
        for b in range(B):
            buf = _padded(target[b:b + 1], H, W, M, dev)
            ar.encode_wavefront(buf, H, W, *_prior_addrs(tp, hp, b, H, W, M), si[0, b], si[1, b])
            if want_y_hat:
                _unpad_into(y_hat, b, buf, H, W)
    if order == "wavefront":
        # one launch gathers symbols and indexes into step order
        sw = torch.empty_like(si)
        F._chk(_lib.hip().stem_ar_to_wave_order(si[0].data_ptr(), si[1].data_ptr(), sw[0].data_ptr(), sw[1].data_ptr(), B, H, W, M, F._stream()))
        si = sw
    sym, idx = si.cpu().numpy()                                                   # one copy of all symbols and indexes

    def code(b):
        enc = BufferedRansEncoder()
        enc.encode_with_indexes(sym[b], idx[b], tables)                        # one host call per image (:955-959); ctypes releases the GIL
        return enc.flush()

    strings = list(_POOL.map(code, range(B))) if B > 1 else [code(0)]
    return (strings, y_hat) if want_y_hat else strings


def stem_decompress(model, strings, shape, y_cond, order="raster"):
    _check_order(order, model)
    _, _, hp, tp = _hyper(model, None, y_cond, strings_z=strings[1], shape=shape)
    yd = F.to_nhwc(y_cond.detach())
    if not model.HAS_SPM:
        scales, means = _one_shot(model, hp, tp)
        return model.gaussian_conditional.decompress(strings[0], None, means=means, scales=scales)
    out = _decode_latents(model, strings[0], hp, tp, order=order)
    if model.RESIDUAL:
        out = F.add(out, _dense(yd))
    return out


def _same_shapes(tensors, what):
    shapes = {tuple(t.shape) for t in tensors}
    if len(shapes) != 1 or next(iter(shapes))[0] != 1:
        raise ValueError(f"{what}: one [1, ...] tensor per chain, all of one size, got {sorted(shapes)}")


def stem_compress_each(model, y_curs, y_conds, order="raster", return_y_hat=False):
    """`stem_compress` of several independent chains (the GOPs evaluation.eval_sequence codes side by side), one [1, M, H, W] pair per
    chain.  The transforms of every chain run at batch 1 -- at another batch size the hyper-prior convolutions may pick another tile /
    split-K plan and move a mean by an ulp, and a stream coded so need not decode at batch 1, which is how a stand-alone decoder runs --
    and only the raster-order coding is batched (`_encode_latents`: its per-image arithmetic is fixed).  -> one result per chain, with
    the keys and the bits `stem_compress` gives for that chain alone (return_y_hat: as there)."""
    _check_order(order, model)
    _same_shapes(list(y_curs) + list(y_conds), "stem_compress_each")
    if not model.HAS_SPM:
        return [stem_compress(model, yc, yd, return_y_hat=return_y_hat) for yc, yd in zip(y_curs, y_conds)]
    zs, hps, tps, targets, yds = [], [], [], [], []
    for y_cur, y_cond in zip(y_curs, y_conds):
        z_strings, zshape, hp, tp = _hyper(model, y_cur, y_cond)
        yc, yd = F.to_nhwc(y_cur.detach()), F.to_nhwc(y_cond.detach())
        targets.append(F.sub(_dense(yc), _dense(yd)) if model.RESIDUAL else _dense(yc))
        zs.append((z_strings, zshape)), hps.append(hp), tps.append(tp), yds.append(yd)
    args = (model, _cat_nhwc(targets), _cat_nhwc(hps), _cat_nhwc(tps) if tps[0] is not None else None, order)
    if not return_y_hat:
        return [_result([y], z, zshape, order) for y, (z, zshape) in zip(_encode_latents(*args), zs)]
    y_strings, rec = _encode_latents(*args, want_y_hat=True)
    return [_result([y], z, zshape, order, _decoded(model, _slice_nhwc(rec, i), yds[i])) for i, (y, (z, zshape)) in enumerate(zip(y_strings, zs))]


def stem_decompress_each(model, strings, shapes, y_conds, order="raster"):
    """`stem_decompress` of several independent chains: strings[i], shapes[i], y_conds[i] are one chain's arguments.  Transforms per chain
    at batch 1, one batched `_decode_latents` call (the concurrent / lockstep routes of `decode_route`).  -> one decoded latent per chain
    (what `stem_decompress` returns: the model's decompress() wraps it)."""
    _check_order(order, model)
    _same_shapes(y_conds, "stem_decompress_each")
    if not model.HAS_SPM:
        return [stem_decompress(model, s, sh, yd) for s, sh, yd in zip(strings, shapes, y_conds)]
    hps, tps = [], []
    for s, sh, y_cond in zip(strings, shapes, y_conds):
        _, _, hp, tp = _hyper(model, None, y_cond, strings_z=s[1], shape=sh)
        hps.append(hp), tps.append(tp)
    out = _decode_latents(model, [s[0][0] for s in strings], _cat_nhwc(hps), _cat_nhwc(tps) if tps[0] is not None else None, order=order)
    res = []
    for i, y_cond in enumerate(y_conds):
        o = _slice_nhwc(out, i)
        res.append(F.add(o, _dense(F.to_nhwc(y_cond.detach()))) if model.RESIDUAL else o)
    return res


_ARP_TRUSTED = {}          # (M, EPM widths, device) -> the persistent decoder reproduced the per-position loop on this process's self-check


def _persistent_trusted(model, M, n0, n1, dev):
    """Once per process, model geometry and device: a 4 x 6 image of synthetic latents is encoded with THIS model's weights and
    decoded twice, by the persistent kernel and by the per-position loop; only if the two agree bit for bit is the persistent
    kernel used from then on.  The kernel's hand-over protocol leans on details a toolchain or driver change can move (a hipcc
    code-generation problem had to be worked around in round 5: csrc/ar_persistent.hip, tools/debug/probe/vec_even_elements.hip;
    32 co-resident workgroups of one XCD are assumed): this is the load-time guard that the parity tests are at build time."""
    key = (M, n0, n1, str(dev))
    if key in _ARP_TRUSTED:
        return _ARP_TRUSTED[key]
    _ARP_TRUSTED[key] = True                               # the check's own decode below takes the persistent route
    try:
        ok = _persistent_selfcheck(model, M, dev)
    except BaseException:
        _ARP_TRUSTED.pop(key, None)                        # nothing was established: the next decode checks again
        raise
    if not ok:
        warnings.warn("the persistent decoder did not reproduce the per-position loop on this process's self-check (toolchain / driver change?): "
                      "decoding with the loop from here on", RuntimeWarning)
    _ARP_TRUSTED[key] = ok
    return ok


def _persistent_selfcheck(model, M, dev):
    H, W = 4, 6
    with torch.no_grad():
        target = _dense(F.to_nhwc(closed_form_input("arp:selfcheck:y", (1, M, H, W), -4.0, 4.0).to(dev)))
        hp = _dense(F.to_nhwc(closed_form_input("arp:selfcheck:hp", (1, 2 * M, H, W), -1.0, 1.0).to(dev)))
        tp = _dense(F.to_nhwc(closed_form_input("arp:selfcheck:tp", (1, 2 * M, H, W), -1.0, 1.0).to(dev))) if model.HAS_TPM else None
        strings = _encode_latents(model, target, hp, tp)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            a = _decode_latents(model, strings, hp, tp).clone()
        b = _decode_latents(model, strings, hp, tp, force_loop=True)
        return bool(torch.equal(a, b)) and not any("persistent decoder gave up" in str(w.message) for w in seen)


def _persistent_ok(model, ar, dev, cfg, force_loop):
    """May the persistent kernel decode for this model?  Asked -- and so self-checked on a geometry's first decode -- whenever the
    configuration would let the kernel run on an image of its own, also when the lockstep loop then takes the batch."""
    n0, n1 = ar.w0.shape[0], ar.w1.shape[0]
    return (cfg.ar_persistent and not force_loop and not cfg.ar_stepwise
            and bool(_lib.hip().stem_ar_decode_image_persistent_supported(ar.M, n0, n1)) and _persistent_trusted(model, ar.M, n0, n1, dev))


def decode_route(B, cfg, persistent_ok, force_loop=False):
    """Which runner of `_Decode` takes a batch of B images under the `ar_*` fields of `cfg` (pure: no library, no device).  `persistent_ok`:
    the kernel supports the model's widths and passed this process's self-check; `force_loop`: that check asking for its reference."""
    if cfg.ar_stepwise:
        return "stepwise"
    if force_loop:
        return "loop"
    persistent = cfg.ar_persistent and persistent_ok
    if B > 1 and persistent and cfg.ar_concurrent and not cfg.ar_force_batch and not cfg.ar_no_batch:
        return "concurrent"
    if (B > 1 or cfg.ar_force_batch) and not cfg.ar_no_batch:
        return "lockstep"
    return "persistent" if persistent else "loop"


def _decode_latents(model, strings_y, hp, tp, force_loop=False, order="raster"):
    """the raster-order decoding of spatiotemporalpriors.py:1015-1054 / priors.py:676-716 for every image of the batch, given the
    hyper prior `hp` (dense NHWC [B, 2M, H, W]) and the temporal prior `tp` (or None) -> the decoded latents, dense NHWC.
    `force_loop`: the per-position loop whatever the configuration prefers (_persistent_selfcheck's reference).  order="wavefront":
    the strings hold their symbols in the order of `wave_order`; one runner decodes them (`_Decode.wave`), `decode_route` is not asked."""
    _check_order(order)
    d = _Decode(model, strings_y, hp, tp)
    if order == "wavefront":
        d.wave()
        return d.out
    cfg = _config.runtime()
    kind = decode_route(d.B, cfg, _persistent_ok(model, d.ar, d.dev, cfg, force_loop), force_loop)
    if kind == "lockstep":
        d.lockstep()
    elif kind == "concurrent":
        for b in d.concurrent():                             # an image whose kernel gave up: once more, alone
            d.persistent(b)
    else:
        for b in range(d.B):
            getattr(d, kind)(b)                              # stepwise, persistent or loop
    return d.out


# one pool for the process (its threads start with the first concurrent decode): the library's per-thread state is allocated once
_POOL = ThreadPoolExecutor(max_workers=8, thread_name_prefix="stem-decode")
_SIDE = {}


class _Decode:
    """One _decode_latents call: the model's loop state, the batch's strings, priors and output, and one runner per kind of decode_route."""

    def __init__(self, model, strings, hp, tp):
        B, P, H, W = hp.shape
        self.strings, self.hp, self.tp = strings, hp, tp
        self.B, self.H, self.W, self.M, self.dev = B, H, W, P // 2, hp.device
        self.ar = _ARContext(model, self.dev)
        self.tables = model.gaussian_conditional.host_tables()
        self.lib = _lib.hip()
        self.out = F.empty_nhwc(B, self.M, H, W, self.dev)
        # host mailbox: pinned (device-visible) memory the index kernel writes and the finish kernel reads directly, so a
        # position costs kernel launches + ONE stream synchronisation and no memcpy calls
        self.idx_host, self.sym_host = (torch.empty(self.M, dtype=torch.int32).pin_memory() for _ in range(2))
        self.decode_fn = C.cast(_lib.rans().stem_rans_decoder_decode, C.c_void_p).value      # host symbol decoder, injected as a C pointer

    def _batched(self, entry, lead):
        """Up to eight images per call of `entry`, a batched decoder of csrc/ar.hip: a zeroed buf, one decoder per image, scratch
        [G, *lead, n] for the four products, pinned mailboxes [G, *lead, M], and the decoded interior into `self.out`."""
        ar, B, H, W, M, dev = self.ar, self.B, self.H, self.W, self.M, self.dev
        for b0 in range(0, B, 8):
            G = min(8, B - b0)
            buf = torch.zeros((G, H + 2 * _P, W + 2 * _P, M), device=dev, dtype=torch.float32)
            scratch = [torch.empty((G, *lead, n), device=dev, dtype=torch.float32) for n in (2 * M, ar.w0.shape[0], ar.w1.shape[0], 2 * M)]
            idx_g, sym_g = (torch.empty((G, *lead, M), dtype=torch.int32).pin_memory() for _ in range(2))
            decs = [_decoder_on(s) for s in self.strings[b0:b0 + G]]
            handles = (C.c_void_p * G)(*[d._h for d in decs])
            F._chk(entry(*ar.net_args(), buf.data_ptr(), G, H, W, M, _P, *_prior_addrs(self.tp, self.hp, b0, H, W, M),
                         *[t.data_ptr() for t in scratch], *ar.table_args(), idx_g.data_ptr(), sym_g.data_ptr(),
                         self.decode_fn, C.addressof(handles), *self.tables.args(), F._stream()))
            self.out[b0:b0 + G].copy_(buf[:, _P:_P + H, _P:_P + W].permute(0, 3, 1, 2))

    def lockstep(self):
        """Independent images advance together (csrc/ar.hip: stem_ar_decode_batch): the loop is bound by the latency of one
        position (4 dependent launches + a host round trip), which G images share; each image's arithmetic is unchanged."""
        self._batched(self.lib.stem_ar_decode_batch, ())

    def wave(self):
        """Wavefront-ordered strings (csrc/ar.hip: stem_ar_decode_wave_batch): W + 3(H-1) steps instead of H * W positions.  A step is
        the encoder's four batched products over the step's positions of up to eight images, one stream synchronisation and one call
        of the host coder per image for the step's np * M symbols, through mailboxes of the largest step's size."""
        self._batched(self.lib.stem_ar_decode_wave_batch, (min(self.H, (self.W + 2) // 3),))

    def stepwise(self, b):
        """The loop of stem_ar_decode_image written with the single-step C-ABI entry points (stem_gemv3_decode, stem_gemv3, stem_ar_finish_decode)
        and the Python RansDecoder: what a host without the fused call would run; the GPU tests check that both produce the same latents."""
        ar, H, W, M = self.ar, self.H, self.W, self.M
        buf, dec = _padded(None, H, W, M, self.dev), _decoder_on(self.strings[b])
        tp_b, hp_b = _prior_addrs(self.tp, self.hp, b, H, W, M)
        Wp = W + 2 * _P
        stream = torch.cuda.current_stream()
        idx, sym = self.idx_host.data_ptr(), self.sym_host.data_ptr()
        idx_np, sym_np = self.idx_host.numpy(), self.sym_host.numpy()
        prev_pix = 0
        for h in range(H):
            for w in range(W):
                pos = h * W + w
                hp_pix = hp_b + 4 * (pos * 2 * M)
                tp_pix = tp_b + 4 * (pos * 2 * M) if tp_b else 0
                if prev_pix and w == 0 and W <= 3:
                    # the previous position (h-1, W-1) is inside this window's rows above: committed first, not folded into the product
                    F._chk(self.lib.stem_ar_finish_decode(ar.gp.data_ptr(), sym, prev_pix, M, F._stream()))
                    prev_pix = 0
                ar.position_decode(buf, Wp, h, w, tp_pix, hp_pix, sym if prev_pix else 0, prev_pix, w > 0, idx)
                stream.synchronize()
                sym_np[:] = dec.decode_stream_np(idx_np, self.tables)
                prev_pix = buf.data_ptr() + 4 * (((h + _P) * Wp + (w + _P)) * M)
        if prev_pix:
            F._chk(self.lib.stem_ar_finish_decode(ar.gp.data_ptr(), sym, prev_pix, M, F._stream()))
        _unpad_into(self.out, b, buf, H, W)

    def loop(self, b):
        """stem_ar_decode_image: four launches + one synchronisation per position (0.29 s per 1080p P frame)"""
        ar, H, W, M = self.ar, self.H, self.W, self.M
        buf, dec = _padded(None, H, W, M, self.dev), _decoder_on(self.strings[b])
        F._chk(self.lib.stem_ar_decode_image(*ar.net_args(), buf.data_ptr(), H, W, M, _P, *_prior_addrs(self.tp, self.hp, b, H, W, M),
                                             *ar.scratch_args(), *ar.table_args(), self.idx_host.data_ptr(), self.sym_host.data_ptr(),
                                             self.decode_fn, dec._h, *self.tables.args(), F._stream()))
        _unpad_into(self.out, b, buf, H, W)

    def persistent_call(self, b, buf, stream):
        """The whole loop of image b as ONE kernel on `stream` (csrc/ar_persistent.hip: 32 resident workgroups of one XCD with the weights
        of their output rows in registers, tagged 8-byte words instead of barriers, the known part of the next position accumulated while
        the host decodes; 0.12-0.13 s per 1080p P frame; bit-identical) -> 0, or an error: a bounded wait ran out, `buf` is half written"""
        ar, H, W, M = self.ar, self.H, self.W, self.M
        dec = _decoder_on(self.strings[b])
        return self.lib.stem_ar_decode_image_persistent(*ar.net_args(), buf.data_ptr(), H, W, M, _P, *_prior_addrs(self.tp, self.hp, b, H, W, M),
                                                        *ar.scratch_args(), *ar.table_args(), self.decode_fn, dec._h, *self.tables.args(), stream)

    def persistent(self, b):
        buf = _padded(None, self.H, self.W, self.M, self.dev)
        if self.persistent_call(b, buf, F._stream()) == 0:
            _unpad_into(self.out, b, buf, self.H, self.W)
        else:
            warnings.warn("persistent decoder gave up (" + (self.lib.stem_last_error() or b"").decode() + "); decoding this image with the per-position loop")
            self.loop(b)                                     # from a fresh buffer and a fresh rANS decoder

    def concurrent(self):
        """One persistent decoder per image, eight at a time (XCD i % 8 for image i): every kernel takes one XCD (32 CUs), its own stream
        and its own host thread for the rANS side (the library keeps its mailboxes per thread); the images do not wait for each other
        as they do in lockstep.  -> the images whose kernel gave up"""
        lib, dev = self.lib, self.dev
        streams = _SIDE.setdefault(dev, [torch.cuda.Stream(device=dev) for _ in range(8)])
        bufs = [_padded(None, self.H, self.W, self.M, dev) for _ in range(self.B)]
        cur = torch.cuda.current_stream(dev)
        for st in streams:
            st.wait_stream(cur)                              # the cleared buffers, tp / hp and the weights are this stream's work

        def work(b):
            torch.cuda.set_device(dev)
            lib.stem_ar_decode_image_persistent_prefer_xcc(b % 8)
            rc = self.persistent_call(b, bufs[b], streams[b % 8].cuda_stream)
            err = (lib.stem_last_error() or b"").decode() if rc else ""
            lib.stem_ar_decode_image_persistent_prefer_xcc(-1)
            return rc, err

        left = []
        for b0 in range(0, self.B, 8):                       # eight XCDs: eight images at a time
            futs = [(b, _POOL.submit(work, b)) for b in range(b0, min(b0 + 8, self.B))]
            for b, f in futs:
                rc, err = f.result()                         # the call returns after its stream has been synchronised
                if rc == 0:
                    _unpad_into(self.out, b, bufs[b], self.H, self.W)
                else:
                    warnings.warn(f"persistent decoder gave up on image {b} ({err}); decoding it with the per-position loop")
                    left.append(b)
        return left


# ---- the I-frame codec: JointAutoregressiveHierarchicalPriors ("mbt2018") --------------------------------------------------------
def iframe_compress(model, x, order="raster", return_y_hat=False):
    """compressai/models/priors.py:544-584: y = g_a(x), z = h_a(y) through the bottleneck's coder, params = h_s(z_hat), then the
    raster-order coding of y itself given params -- the same loop as a STEM model without temporal prior and without residual"""
    _check_order(order, model)
    eb = model.entropy_bottleneck
    y = model.g_a(x)
    z = model.h_a(y)
    z_strings = eb.compress(z)
    z_hat = eb.decompress(z_strings, z.shape[-2:]).to(y.device).float()
    params = _dense(F.to_nhwc(model.h_s(z_hat)))
    yn = _dense(F.to_nhwc(y.detach()))
    _check_latent_size(yn, params, "images")
    if not return_y_hat:
        return _result(_encode_latents(model, yn, params, None, order), z_strings, z.shape[-2:], order)
    y_strings, y_hat = _encode_latents(model, yn, params, None, order, want_y_hat=True)       # "y_hat": what iframe_decompress returns as "y_hat"
    return _result(y_strings, z_strings, z.shape[-2:], order, y_hat)


def iframe_decompress(model, strings, shape, order="raster"):
    """compressai/models/priors.py:633-674 -> {"x_hat", "y_hat"}"""
    _check_order(order, model)
    assert isinstance(strings, list) and len(strings) == 2
    z_hat = model.entropy_bottleneck.decompress(strings[1], shape)
    dev = next(model.parameters()).device
    params = _dense(F.to_nhwc(model.h_s(z_hat.to(dev).float())))
    y_hat = _decode_latents(model, strings[0], params, None, order=order)
    x_hat = F.to_nchw(model.g_s(y_hat), clamp01=True)
    return {"x_hat": x_hat, "y_hat": y_hat}


def iframe_compress_each(model, xs, order="raster", return_y_hat=False):
    """`iframe_compress` of several independent images, one [1, 3, h, w] tensor each: g_a, h_a, h_s per image at batch 1 (see
    `stem_compress_each`), one batched raster-order coding.  -> one result per image, the bits of `iframe_compress` of it alone."""
    _check_order(order, model)
    _same_shapes(xs, "iframe_compress_each")
    eb = model.entropy_bottleneck
    zs, ys, params = [], [], []
    for x in xs:
        y = model.g_a(x)
        z = model.h_a(y)
        z_strings = eb.compress(z)
        z_hat = eb.decompress(z_strings, z.shape[-2:]).to(y.device).float()
        p = _dense(F.to_nhwc(model.h_s(z_hat)))
        yn = _dense(F.to_nhwc(y.detach()))
        _check_latent_size(yn, p, "images")
        zs.append((z_strings, z.shape[-2:])), ys.append(yn), params.append(p)
    if not return_y_hat:
        y_strings = _encode_latents(model, _cat_nhwc(ys), _cat_nhwc(params), None, order)
        return [_result([y], z, zshape, order) for y, (z, zshape) in zip(y_strings, zs)]
    y_strings, y_hats = _encode_latents(model, _cat_nhwc(ys), _cat_nhwc(params), None, order, want_y_hat=True)
    return [_result([y], z, zshape, order, _slice_nhwc(y_hats, i)) for i, (y, (z, zshape)) in enumerate(zip(y_strings, zs))]


def iframe_decompress_each(model, strings, shapes, order="raster", latents_only=False):
    """`iframe_decompress` of several independent images: h_s and g_s per image at batch 1, one batched `_decode_latents` call.
    -> one {"x_hat", "y_hat"} per image; latents_only=True: {"y_hat"} alone, g_s does not run (video.verify_sequence)."""
    _check_order(order, model)
    dev = next(model.parameters()).device
    params = []
    for s, sh in zip(strings, shapes):
        assert isinstance(s, list) and len(s) == 2
        z_hat = model.entropy_bottleneck.decompress(s[1], sh)
        params.append(_dense(F.to_nhwc(model.h_s(z_hat.to(dev).float()))))
    _same_shapes(params, "iframe_decompress_each")
    y_hats = _decode_latents(model, [s[0][0] for s in strings], _cat_nhwc(params), None, order=order)
    res = []
    for i in range(len(params)):
        y_hat = _slice_nhwc(y_hats, i)
        res.append({"y_hat": y_hat} if latents_only else {"x_hat": F.to_nchw(model.g_s(y_hat), clamp01=True), "y_hat": y_hat})
    return res


def _cat_nhwc(ts):
    """dense NHWC [1, C, H, W] tensors -> one dense NHWC [len, C, H, W] (a copy per image, no arithmetic)"""
    if len(ts) == 1:
        return ts[0]
    _, Cn, H, W = ts[0].shape
    out = F.empty_nhwc(len(ts), Cn, H, W, ts[0].device)
    for i, t in enumerate(ts):
        out[i:i + 1].copy_(t)
    return out


def _slice_nhwc(t, i):
    """image i of a dense NHWC batch as a dense NHWC [1, C, H, W] tensor of its own"""
    if t.shape[0] == 1:
        return t
    out = F.empty_nhwc(1, *t.shape[1:], t.device)
    out.copy_(t[i:i + 1])
    return out


def _dense(t):
    if F.nhwc_ld(t) != t.shape[1]:
        t = F.copy_channels(t, F.empty_nhwc(*t.shape, t.device))
    return t
