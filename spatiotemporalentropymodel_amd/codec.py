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
0.74 s vs 0.44 s per 1080p frame.  One image: a persistent kernel, csrc/ar_persistent.hip.)
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import config as _config
from . import functional as F
from .entropy_models import BufferedRansEncoder, RansDecoder

_K = 5      # context kernel size
_P = 2      # its padding


def _hyper(model, y_cur, y_cond, strings_z=None, shape=None):
    """z path shared by compress / decompress: returns (z_strings, hp, tp) with hp/tp dense NHWC tensors."""
    eng = model.engine()
    eb = model.entropy_bottleneck
    yd = F.to_nhwc(y_cond.detach())
    if strings_z is None:
        yc = F.to_nhwc(y_cur.detach())
        B, Cin, H, W = yc.shape
        he_in = F.empty_nhwc(B, 2 * Cin, H, W, yc.device)
        F.copy_channels(yc, he_in[:, :Cin])
        F.copy_channels(yd, he_in[:, Cin:])
        z = eng.HE[2].fwd(eng.HE[1].fwd(eng.HE[0].fwd(he_in, F.ACT_LRELU), F.ACT_LRELU))
        strings_z = eb.compress(z)
        shape = z.shape[-2:]
    z_hat = eb.decompress(strings_z, shape).to(yd.device).float()
    hp = eng.HD[2].fwd(eng.HD[1].fwd(eng.HD[0].fwd(F.to_nhwc(z_hat), F.ACT_LRELU), F.ACT_LRELU))
    if tuple(hp.shape[-2:]) != tuple(yd.shape[-2:]):
        raise ValueError(f"latent size {tuple(yd.shape[-2:])} does not survive the two stride-2 hyper stages (hyper-prior is "
                         f"{tuple(hp.shape[-2:])}): pad frames to multiples of 64 pixels, as stem/evalSTEM.py:95-108 does")
    tp = None
    if eng.has_tpm:
        tp = eng.TPM[2].fwd(eng.TPM[1].fwd(eng.TPM[0].fwd(yd, F.ACT_LRELU), F.ACT_LRELU))
    return strings_z, shape, hp, tp


def _gaussian_params(model, priors):
    """EPM on the concatenated priors (all dense NHWC) -> gp = scales | means."""
    eng = model.engine()
    B, P, H, W = priors[0].shape
    epm_in = F.empty_nhwc(B, P * len(priors), H, W, priors[0].device)
    for i, p in enumerate(priors):
        F.copy_channels(p, epm_in[:, i * P:(i + 1) * P])
    return eng.EPM[2].fwd(eng.EPM[1].fwd(eng.EPM[0].fwd(epm_in, F.ACT_LRELU), F.ACT_LRELU))


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
        self.w0 = m.EPM[0].weight.detach().reshape(m.EPM[0].out_channels, -1).contiguous()
        self.w1 = m.EPM[2].weight.detach().reshape(m.EPM[2].out_channels, -1).contiguous()
        self.w2 = m.EPM[4].weight.detach().reshape(m.EPM[4].out_channels, -1).contiguous()
        self.b0, self.b1, self.b2 = m.EPM[0].bias.detach(), m.EPM[2].bias.detach(), m.EPM[4].bias.detach()
        self.ctx = torch.empty(2 * M, device=device)
        self.h1 = torch.empty(self.w0.shape[0], device=device)
        self.h2 = torch.empty(self.w1.shape[0], device=device)
        self.gp = torch.empty(2 * M, device=device)
        self.table = m.gaussian_conditional.scale_table.to(device).float().contiguous()
        self.bound = m.gaussian_conditional._scale_bound
        self.has_tpm = m.HAS_TPM

    def encode_wavefront(self, buf, H, W, tp_b, hp_b, sym, idx):
        """All positions with equal t = w + 3h are independent under the 5x5 type-A mask: W + 3(H-1) batched steps
        (csrc/ar.hip) instead of H*W sequential ones; symbols / indexes are written in raster order."""
        lib, M, st = _lib.hip(), self.M, F._stream()
        P, Wp = 2 * M, W + 2 * _P
        npmax = min(H, (W + 2) // 3)
        dev = buf.device
        if getattr(self, "_wave_np", 0) < npmax:
            self._wctx = torch.empty((npmax, P), device=dev)
            self._wh1 = torch.empty((npmax, self.w0.shape[0]), device=dev)
            self._wh2 = torch.empty((npmax, self.w1.shape[0]), device=dev)
            self._wgp = torch.empty((npmax, P), device=dev)
            self._wave_np = npmax
        if not _config.runtime().ar_stepwise:
            # all W + 3(H-1) steps queued by one library call (no interpreter between the 5 launches of a step)
            F._chk(lib.stem_ar_encode_image(
                self.w_ctx.data_ptr(), 12 * M, self.b_ctx.data_ptr(), self.w0.data_ptr(), self.w0.shape[1], self.b0.data_ptr(), self.w0.shape[0],
                self.w1.data_ptr(), self.w1.shape[1], self.b1.data_ptr(), self.w1.shape[0], self.w2.data_ptr(), self.w2.shape[1], self.b2.data_ptr(),
                buf.data_ptr(), H, W, M, _P, tp_b, hp_b, self._wctx.data_ptr(), self._wh1.data_ptr(), self._wh2.data_ptr(), self._wgp.data_ptr(),
                self.table.data_ptr(), self.table.numel(), self.bound, F.LRELU_SLOPE, sym.data_ptr(), idx.data_ptr(), st))
            return
        S = _lib.WaveSeg
        base = buf.data_ptr()
        row = Wp * M
        seg_ctx = (S * 3)(S(base, 5 * M, 0, row, M, 0), S(base + 4 * row, 5 * M, 5 * M, row, M, 0), S(base + 8 * row, 2 * M, 10 * M, row, M, 0))
        ctx_seg = S(self._wctx.data_ptr(), P, 0, 0, 0, P)
        if self.has_tpm:
            ctx_seg.woff = 2 * P
            seg_e0 = (S * 3)(S(tp_b, P, 0, W * P, P, 0), S(hp_b, P, P, W * P, P, 0), ctx_seg)
        else:
            ctx_seg.woff = P
            seg_e0 = (S * 3)(S(hp_b, P, 0, W * P, P, 0), ctx_seg, S(0, 0, 0, 0, 0, 0))
        n1, n2 = self.w0.shape[0], self.w1.shape[0]
        seg_e1 = (S * 3)(S(self._wh1.data_ptr(), n1, 0, 0, 0, n1), S(0, 0, 0, 0, 0, 0), S(0, 0, 0, 0, 0, 0))
        seg_e2 = (S * 3)(S(self._wh2.data_ptr(), n2, 0, 0, 0, n2), S(0, 0, 0, 0, 0, 0), S(0, 0, 0, 0, 0, 0))
        import ctypes as C
        a_ctx, a_e0, a_e1, a_e2 = (C.addressof(x) for x in (seg_ctx, seg_e0, seg_e1, seg_e2))
        for t in range(W + 3 * (H - 1)):
            F._chk(lib.stem_gemv3_wave(self.w_ctx.data_ptr(), 12 * M, self.b_ctx.data_ptr(), a_ctx, self._wctx.data_ptr(), P, P, 0, 0.0, t, H, W, st))
            F._chk(lib.stem_gemv3_wave(self.w0.data_ptr(), self.w0.shape[1], self.b0.data_ptr(), a_e0, self._wh1.data_ptr(), n1, n1,
                                       F.ACT_LRELU, F.LRELU_SLOPE, t, H, W, st))
            F._chk(lib.stem_gemv3_wave(self.w1.data_ptr(), self.w1.shape[1], self.b1.data_ptr(), a_e1, self._wh2.data_ptr(), n2, n2,
                                       F.ACT_LRELU, F.LRELU_SLOPE, t, H, W, st))
            F._chk(lib.stem_gemv3_wave(self.w2.data_ptr(), self.w2.shape[1], self.b2.data_ptr(), a_e2, self._wgp.data_ptr(), P, P, 0, 0.0, t, H, W, st))
            F._chk(lib.stem_ar_finish_encode_wave(self._wgp.data_ptr(), self.table.data_ptr(), self.table.numel(), self.bound,
                                                  buf.data_ptr(), sym.data_ptr(), idx.data_ptr(), M, t, H, W, Wp, _P, st))


def _position_decode(self, buf, Wp, h, w, tp_pix, hp_pix, sym_prev, pix_prev, prev_is_left, idx_out):
    """Decoder form of _ARContext.position: the first product also writes back the previous position's y_hat (and uses it
    in place of the not-yet-visible left neighbour), the last one also emits the CDF indexes."""
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


_ARContext.position_decode = _position_decode


def decode_image_stepwise(ar, buf, H, W, tp_b, hp_b, dec, tables, idx_host, sym_host):
    """The loop of stem_ar_decode_image written with the single-step C-ABI entry points (stem_gemv3_decode, stem_gemv3,
    stem_ar_finish_decode) and the Python RansDecoder: what a host without the fused call would run; the GPU tests check
    that both produce the same latents."""
    lib, M = _lib.hip(), ar.M
    Wp = W + 2 * _P
    stream = torch.cuda.current_stream()
    idx_np, sym_np = idx_host.numpy(), sym_host.numpy()
    prev_pix = 0
    for h in range(H):
        for w in range(W):
            pos = h * W + w
            hp_pix = hp_b + 4 * (pos * 2 * M)
            tp_pix = tp_b + 4 * (pos * 2 * M) if tp_b else 0
            ar.position_decode(buf, Wp, h, w, tp_pix, hp_pix, sym_host.data_ptr() if prev_pix else 0, prev_pix, w > 0, idx_host.data_ptr())
            stream.synchronize()
            sym_np[:] = dec.decode_stream_np(idx_np, tables)
            prev_pix = buf.data_ptr() + 4 * (((h + _P) * Wp + (w + _P)) * M)
    if prev_pix:
        F._chk(lib.stem_ar_finish_decode(ar.gp.data_ptr(), sym_host.data_ptr(), prev_pix, M, F._stream()))


def _padded(target_img, H, W, M, device):
    """[Hp, Wp, M] zero-padded NHWC copy of one image's latent (F.pad(..., (2,2,2,2)), :898)."""
    buf = torch.zeros((H + 2 * _P, W + 2 * _P, M), device=device, dtype=torch.float32)
    if target_img is not None:
        inner = buf[_P:_P + H, _P:_P + W].permute(2, 0, 1).unsqueeze(0)          # [1,M,H,W] view, pitch-strided rows
        inner.copy_(target_img)                                                   # one small strided copy per image
    return buf


def stem_compress(model, y_cur, y_cond):
    gc = model.gaussian_conditional
    z_strings, zshape, hp, tp = _hyper(model, y_cur, y_cond)
    yc, yd = F.to_nhwc(y_cur.detach()), F.to_nhwc(y_cond.detach())
    B, M, H, W = yc.shape
    target = F.sub(_dense(yc), _dense(yd)) if model.RESIDUAL else _dense(yc)
    if not model.HAS_SPM:
        gp = _gaussian_params(model, [p for p in (tp, hp) if p is not None])
        scales, means = gp[:, :M], gp[:, M:]
        indexes = gc.build_indexes(scales)
        y_strings = gc.compress(target, indexes, means=means)
        return {"strings": [y_strings, z_strings], "shape": zshape}
    return {"strings": [_encode_latents(model, target, hp, tp), z_strings], "shape": zshape}


def _encode_latents(model, target, hp, tp):
    """the raster-order coding of `target` (dense NHWC [B, M, H, W]) given the hyper prior `hp` and the temporal prior `tp` (or
    None): spatiotemporalpriors.py:916-961 / priors.py:586-631 -> one string per image"""
    gc = model.gaussian_conditional
    B, M, H, W = target.shape
    dev = target.device
    ar = _ARContext(model, dev)
    tables = gc.host_tables()
    y_strings = []
    for b in range(B):
        buf = _padded(target[b:b + 1], H, W, M, dev)
        sym = torch.empty((H * W, M), device=dev, dtype=torch.int32)
        idx = torch.empty((H * W, M), device=dev, dtype=torch.int32)
        hp_b = hp.data_ptr() + 4 * (b * H * W * 2 * M)
        tp_b = tp.data_ptr() + 4 * (b * H * W * 2 * M) if tp is not None else 0
        ar.encode_wavefront(buf, H, W, tp_b, hp_b, sym, idx)
        enc = BufferedRansEncoder()
        enc.encode_with_indexes(sym.cpu().numpy(), idx.cpu().numpy(), tables)      # one host call per image (:955-959)
        y_strings.append(enc.flush())
    return y_strings


def stem_decompress(model, strings, shape, y_cond):
    gc = model.gaussian_conditional
    _, _, hp, tp = _hyper(model, None, y_cond, strings_z=strings[1], shape=shape)
    yd = F.to_nhwc(y_cond.detach())
    B, P, H, W = hp.shape
    M = P // 2
    if not model.HAS_SPM:
        gp = _gaussian_params(model, [p for p in (tp, hp) if p is not None])
        scales, means = gp[:, :M], gp[:, M:]
        indexes = gc.build_indexes(scales)
        return gc.decompress(strings[0], indexes, means=means)
    out = _decode_latents(model, strings[0], hp, tp)
    if model.RESIDUAL:
        out = F.add(out, _dense(yd))
    return out


_ARP_TRUSTED = {}          # (M, EPM widths, device) -> the persistent decoder reproduced the per-position loop on this process's self-check
_FORCE_LOOP = False


def _persistent_trusted(model, M, n0, n1, dev):
    """Once per process, model geometry and device: a 4 x 6 image of synthetic latents is encoded with THIS model's weights and
    decoded twice, by the persistent kernel and by the per-position loop; only if the two agree bit for bit is the persistent
    kernel used from then on.  The kernel's hand-over protocol leans on details a toolchain or driver change can move (a hipcc
    code-generation problem had to be worked around in round 5: csrc/ar_persistent.hip, tools/debug/probe/vec_even_elements.hip;
    32 co-resident workgroups of one XCD are assumed): this is the load-time guard that the parity tests are at build time."""
    global _FORCE_LOOP
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
        import warnings
        warnings.warn("the persistent decoder did not reproduce the per-position loop on this process's self-check (toolchain / driver change?): "
                      "decoding with the loop from here on", RuntimeWarning)
    _ARP_TRUSTED[key] = ok
    return ok


def _persistent_selfcheck(model, M, dev):
    global _FORCE_LOOP
    from .weights import closed_form_input
    H, W = 4, 6
    with torch.no_grad():
        target = _dense(F.to_nhwc(closed_form_input("arp:selfcheck:y", (1, M, H, W), -4.0, 4.0).to(dev)))
        hp = _dense(F.to_nhwc(closed_form_input("arp:selfcheck:hp", (1, 2 * M, H, W), -1.0, 1.0).to(dev)))
        tp = _dense(F.to_nhwc(closed_form_input("arp:selfcheck:tp", (1, 2 * M, H, W), -1.0, 1.0).to(dev))) if model.HAS_TPM else None
        strings = _encode_latents(model, target, hp, tp)
        import warnings
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            a = _decode_latents(model, strings, hp, tp).clone()
        _FORCE_LOOP = True
        try:
            b = _decode_latents(model, strings, hp, tp)
        finally:
            _FORCE_LOOP = False
        return bool(torch.equal(a, b)) and not any("persistent decoder gave up" in str(w.message) for w in seen)


def _decode_latents(model, strings_y, hp, tp):
    """the raster-order decoding of spatiotemporalpriors.py:1015-1054 / priors.py:676-716 for every image of the batch, given the
    hyper prior `hp` (dense NHWC [B, 2M, H, W]) and the temporal prior `tp` (or None) -> the decoded latents, dense NHWC"""
    gc = model.gaussian_conditional
    strings = [strings_y]
    B, P, H, W = hp.shape
    M = P // 2
    dev = hp.device
    ar = _ARContext(model, dev)
    tables = gc.host_tables()
    lib = _lib.hip()
    Wp = W + 2 * _P
    out = F.empty_nhwc(B, M, H, W, dev)
    # host mailbox: pinned (device-visible) memory the index kernel writes and the finish kernel reads directly, so a
    # position costs kernel launches + ONE stream synchronisation and no memcpy calls
    idx_host = torch.empty(M, dtype=torch.int32).pin_memory()
    sym_host = torch.empty(M, dtype=torch.int32).pin_memory()
    import ctypes as C
    decode_fn = C.cast(_lib.rans().stem_rans_decoder_decode, C.c_void_p).value      # host symbol decoder, injected as a C pointer
    cfg = _config.runtime()
    stepwise = cfg.ar_stepwise
    lockstep = (B > 1 or cfg.ar_force_batch) and not stepwise and not cfg.ar_no_batch
    decoded = set()
    persistent = (cfg.ar_persistent and not _FORCE_LOOP and not stepwise
                  and bool(lib.stem_ar_decode_image_persistent_supported(M, ar.w0.shape[0], ar.w1.shape[0]))
                  and _persistent_trusted(model, M, ar.w0.shape[0], ar.w1.shape[0], dev))
    if _FORCE_LOOP:
        lockstep = False
    if B > 1 and persistent and cfg.ar_concurrent and not cfg.ar_force_batch and not cfg.ar_no_batch:
        # Several images: one persistent decoder each, eight at a time -- every kernel takes one XCD (32 CUs), its own stream and its own
        # host thread for the rANS side (the library keeps its mailboxes per thread); the images do not wait for each other as they
        # do in the lockstep loop below.  An image whose kernel gives up is decoded by the per-position loop further down.
        decoded = _decode_concurrently(lib, ar, strings[0], out, H, W, M, tp, hp, tables, decode_fn, dev)
        lockstep = False
    if lockstep:
        # Independent images advance together (csrc/ar.hip: stem_ar_decode_batch): the loop is bound by the latency of one
        # position (4 dependent launches + a host round trip), which G images share; each image's arithmetic is unchanged.
        GMAX = 8
        for b0 in range(0, B, GMAX):
            G = min(GMAX, B - b0)
            buf = torch.zeros((G, H + 2 * _P, Wp, M), device=dev, dtype=torch.float32)
            scratch = [torch.empty((G, n), device=dev, dtype=torch.float32) for n in (2 * M, ar.w0.shape[0], ar.w1.shape[0], 2 * M)]
            idx_g = torch.empty((G, M), dtype=torch.int32).pin_memory()
            sym_g = torch.empty((G, M), dtype=torch.int32).pin_memory()
            decs = []
            for s in strings[0][b0:b0 + G]:
                d = RansDecoder()
                d.set_stream(s)
                decs.append(d)
            handles = (C.c_void_p * G)(*[d._h for d in decs])
            hp_b = hp.data_ptr() + 4 * (b0 * H * W * 2 * M)
            tp_b = tp.data_ptr() + 4 * (b0 * H * W * 2 * M) if tp is not None else 0
            common = (ar.w_ctx.data_ptr(), 12 * M, ar.b_ctx.data_ptr(), ar.w0.data_ptr(), ar.w0.shape[1], ar.b0.data_ptr(), ar.w0.shape[0],
                      ar.w1.data_ptr(), ar.w1.shape[1], ar.b1.data_ptr(), ar.w1.shape[0], ar.w2.data_ptr(), ar.w2.shape[1], ar.b2.data_ptr(),
                      buf.data_ptr(), G, H, W, M, _P, tp_b, hp_b, *[t.data_ptr() for t in scratch],
                      ar.table.data_ptr(), ar.table.numel(), ar.bound, F.LRELU_SLOPE)
            F._chk(lib.stem_ar_decode_batch(*common, idx_g.data_ptr(), sym_g.data_ptr(), decode_fn, C.addressof(handles),
                                            *tables.args(), F._stream()))
            out[b0:b0 + G].copy_(buf[:, _P:_P + H, _P:_P + W].permute(0, 3, 1, 2))
    for b, s in enumerate(strings[0] if not lockstep else []):
        if b in decoded:
            continue
        buf = _padded(None, H, W, M, dev)
        dec = RansDecoder()
        dec.set_stream(s)
        hp_b = hp.data_ptr() + 4 * (b * H * W * 2 * M)
        tp_b = tp.data_ptr() + 4 * (b * H * W * 2 * M) if tp is not None else 0
        if stepwise:                                          # same loop from Python with the single-step entry points (tests)
            decode_image_stepwise(ar, buf, H, W, tp_b, hp_b, dec, tables, idx_host, sym_host)
            out[b:b + 1].copy_(buf[_P:_P + H, _P:_P + W].permute(2, 0, 1).unsqueeze(0))
            continue
        # The whole raster-order loop of this image runs inside the library: as ONE persistent kernel (csrc/ar_persistent.hip: 32 resident
        # workgroups of one XCD with the weights of their output rows in registers, tagged 8-byte words instead of barriers, the known
        # part of the next position accumulated while the host decodes; 0.12-0.13 s per 1080p P frame) or, STEM_AR_PERSISTENT=0 /
        # unsupported widths / a bounded wait that ran out, as four launches + one synchronisation per position (0.29 s).  Bit-identical.
        if persistent:
            rc = lib.stem_ar_decode_image_persistent(
                ar.w_ctx.data_ptr(), 12 * M, ar.b_ctx.data_ptr(), ar.w0.data_ptr(), ar.w0.shape[1], ar.b0.data_ptr(), ar.w0.shape[0],
                ar.w1.data_ptr(), ar.w1.shape[1], ar.b1.data_ptr(), ar.w1.shape[0], ar.w2.data_ptr(), ar.w2.shape[1], ar.b2.data_ptr(),
                buf.data_ptr(), H, W, M, _P, tp_b, hp_b, ar.ctx.data_ptr(), ar.h1.data_ptr(), ar.h2.data_ptr(), ar.gp.data_ptr(),
                ar.table.data_ptr(), ar.table.numel(), ar.bound, F.LRELU_SLOPE, decode_fn, dec._h, *tables.args(), F._stream())
            if rc == 0:
                out[b:b + 1].copy_(buf[_P:_P + H, _P:_P + W].permute(2, 0, 1).unsqueeze(0))
                continue
            import warnings
            warnings.warn("persistent decoder gave up (" + (lib.stem_last_error() or b"").decode() + "); decoding this image with the per-position loop")
            buf = _padded(None, H, W, M, dev)
            dec = RansDecoder()
            dec.set_stream(s)
        F._chk(lib.stem_ar_decode_image(
            ar.w_ctx.data_ptr(), 12 * M, ar.b_ctx.data_ptr(), ar.w0.data_ptr(), ar.w0.shape[1], ar.b0.data_ptr(), ar.w0.shape[0],
            ar.w1.data_ptr(), ar.w1.shape[1], ar.b1.data_ptr(), ar.w1.shape[0], ar.w2.data_ptr(), ar.w2.shape[1], ar.b2.data_ptr(),
            buf.data_ptr(), H, W, M, _P, tp_b, hp_b, ar.ctx.data_ptr(), ar.h1.data_ptr(), ar.h2.data_ptr(), ar.gp.data_ptr(),
            ar.table.data_ptr(), ar.table.numel(), ar.bound, F.LRELU_SLOPE, idx_host.data_ptr(), sym_host.data_ptr(),
            decode_fn, dec._h, *tables.args(), F._stream()))
        out[b:b + 1].copy_(buf[_P:_P + H, _P:_P + W].permute(2, 0, 1).unsqueeze(0))
    return out


# ---- the I-frame codec: JointAutoregressiveHierarchicalPriors ("mbt2018") --------------------------------------------------------
def iframe_compress(model, x):
    """compressai/models/priors.py:544-584: y = g_a(x), z = h_a(y) through the bottleneck's coder, params = h_s(z_hat), then the
    raster-order coding of y itself given params -- the same loop as a STEM model without temporal prior and without residual"""
    eb = model.entropy_bottleneck
    y = model.g_a(x)
    z = model.h_a(y)
    z_strings = eb.compress(z)
    z_hat = eb.decompress(z_strings, z.shape[-2:]).to(y.device).float()
    params = _dense(F.to_nhwc(model.h_s(z_hat)))
    yn = _dense(F.to_nhwc(y.detach()))
    if tuple(params.shape[-2:]) != tuple(yn.shape[-2:]):
        raise ValueError(f"latent size {tuple(yn.shape[-2:])} does not survive the two stride-2 hyper stages (hyper-prior is "
                         f"{tuple(params.shape[-2:])}): pad images to multiples of 64 pixels, as stem/evalSTEM.py:95-108 does")
    return {"strings": [_encode_latents(model, yn, params, None), z_strings], "shape": z.shape[-2:]}


def iframe_decompress(model, strings, shape):
    """compressai/models/priors.py:633-674 -> {"x_hat", "y_hat"}"""
    assert isinstance(strings, list) and len(strings) == 2
    z_hat = model.entropy_bottleneck.decompress(strings[1], shape)
    dev = next(model.parameters()).device
    params = _dense(F.to_nhwc(model.h_s(z_hat.to(dev).float())))
    y_hat = _decode_latents(model, strings[0], params, None)
    x_hat = F.to_nchw(model.g_s(y_hat), clamp01=True)
    return {"x_hat": x_hat, "y_hat": y_hat}


_POOL = None
_SIDE = {}


def _decode_concurrently(lib, ar, strings_y, out, H, W, M, tp, hp, tables, decode_fn, dev):
    """stem_ar_decode_image_persistent for images 0 .. B-1, up to eight at once (XCD i % 8 for image i) -> the set of images done"""
    global _POOL
    import warnings
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=8, thread_name_prefix="stem-decode")     # kept: the library's per-thread state is allocated once
    streams = _SIDE.setdefault(dev, [torch.cuda.Stream(device=dev) for _ in range(8)])
    B = len(strings_y)
    bufs = [_padded(None, H, W, M, dev) for _ in range(B)]
    cur = torch.cuda.current_stream(dev)
    for st in streams:
        st.wait_stream(cur)                                  # the cleared buffers, tp / hp and the weights are this stream's work

    def job(b):
        torch.cuda.set_device(dev)
        lib.stem_ar_decode_image_persistent_prefer_xcc(b % 8)
        dec = RansDecoder()
        dec.set_stream(strings_y[b])
        hp_b = hp.data_ptr() + 4 * (b * H * W * 2 * M)
        tp_b = tp.data_ptr() + 4 * (b * H * W * 2 * M) if tp is not None else 0
        rc = lib.stem_ar_decode_image_persistent(
            ar.w_ctx.data_ptr(), 12 * M, ar.b_ctx.data_ptr(), ar.w0.data_ptr(), ar.w0.shape[1], ar.b0.data_ptr(), ar.w0.shape[0],
            ar.w1.data_ptr(), ar.w1.shape[1], ar.b1.data_ptr(), ar.w1.shape[0], ar.w2.data_ptr(), ar.w2.shape[1], ar.b2.data_ptr(),
            bufs[b].data_ptr(), H, W, M, _P, tp_b, hp_b, ar.ctx.data_ptr(), ar.h1.data_ptr(), ar.h2.data_ptr(), ar.gp.data_ptr(),
            ar.table.data_ptr(), ar.table.numel(), ar.bound, F.LRELU_SLOPE, decode_fn, dec._h, *tables.args(), streams[b % 8].cuda_stream)
        err = (lib.stem_last_error() or b"").decode() if rc else ""
        lib.stem_ar_decode_image_persistent_prefer_xcc(-1)
        return rc, err

    done = set()
    for b0 in range(0, B, 8):                                # eight XCDs: eight images at a time
        futs = [(b, _POOL.submit(job, b)) for b in range(b0, min(b0 + 8, B))]
        for b, f in futs:
            rc, err = f.result()                             # the call returns after its stream has been synchronised
            if rc == 0:
                out[b:b + 1].copy_(bufs[b][_P:_P + H, _P:_P + W].permute(2, 0, 1).unsqueeze(0))
                done.add(b)
            else:
                warnings.warn(f"persistent decoder gave up on image {b} ({err}); decoding it with the per-position loop")
    return done


def _dense(t):
    if F.nhwc_ld(t) != t.shape[1]:
        t = F.copy_channels(t, F.empty_nhwc(*t.shape, t.device))
    return t
