"""Layer modules with the reference's names, constructor arguments and state-dict keys, whose forward/backward run the HIP
kernels through the C ABI -- and the one place that decides which kernel family serves a convolution (`route`).

  Conv2d / ConvTranspose2d   torch.nn.Conv2d / ConvTranspose2d as built by compressai/models/utils.py:112-130 (conv / deconv)
  MaskedConv2d, GDN, GDN1    compressai/layers/layers.py:21-47, gdn.py:22-96;  LeakyReLU: index-keeping placeholder
  FusedSequential            nn.Sequential that plans its children into steps (conv, conv+GDN, conv+LeakyReLU), then runs them
  route / Route / Step       the kernel family of a convolution as a value; f16x3_same_shape: the shape rule engine.py shares
  cat / to_nchw / adaptive_avg_pool2d, the *Function classes      glue operations of the layer-wise models (stem_utils.py, stem_roi.py)
  bump_weight_epoch / weight_epoch / wgrad_side_stream / join_wgrad_stream      what optimisers and trainers synchronise with
  PixelShuffleFunction / AddActFunction / GateFunction, and (re-exported from layers_residual.py) conv3x3, conv1x1, subpel_conv3x3,
  ResidualBlock*, AttentionBlock, BlockSequential      the blocks of the cheng2020 models, compressai/layers/layers.py:50-213
"""
from __future__ import annotations

import collections
import math

import torch
import torch.nn as nn

from . import config as _config
from . import functional as F
from .ops import NonNegativeParametrizer

_WEIGHT_EPOCH = [0]


def bump_weight_epoch(params=None):
    """Called by the fused optimiser: parameters changed behind torch's version counters.  With `params` only those
    tensors are marked (each carries its own counter), so packed copies of other models' weights -- e.g. the frozen
    I-frame transforms next to a training STEM -- stay valid; without, every cache is invalidated."""
    if params is None:
        _WEIGHT_EPOCH[0] += 1
        return
    for p in params:
        p._stem_epoch = getattr(p, "_stem_epoch", 0) + 1


def weight_epoch(w):
    return (_WEIGHT_EPOCH[0], getattr(w, "_stem_epoch", 0))


PACK_F16X2 = -3          # _PackCache role of the pre-split fp16 image (csrc/conv_f16x3.hip); not a stem_pack_* role
PACK_F16X2_GEN = -4      # ... in the layout of the general (128-column tiles, split-K) kernel
PACK_F16X2_FLIP = -7     # PACK_F16X2 of the mirrored, transposed weight (input gradient on the 192-column kernel)
PACK_F16X2_GEN_FLIP = -6 # ... of the mirrored, transposed weight: the input-gradient of a stride-1 convolution as a convolution
PACK_C4GDN = -5           # A-operand stream of csrc/c4gdn_f16x3.hip: first-layer weight AND the following GDN's gamma
PACK_GDN_GAMMA = -8       # reparametrised gamma of the GDN fused into conv_f16x3_kernel, packed as a 1x1 weight image

#: role -> packer, for the roles above (every other role is a stem_pack_* role: F.pack_weight(w, role, masked))
_PACKERS = {
    PACK_F16X2: F.pack_weight_f16x2,
    PACK_F16X2_FLIP: lambda w: F.pack_weight_f16x2(w, flip=True),
    PACK_F16X2_GEN: F.pack_weight_f16x2_gen,
    PACK_F16X2_GEN_FLIP: lambda w: F.pack_weight_f16x2_gen(w, flip=True),
    PACK_GDN_GAMMA: F.pack_gdn_gamma_f16x2,
}


class _PackCache:
    """Packed weight copies, rebuilt only when the parameter changed."""

    def __init__(self):
        self._c = {}

    def _cached(self, role, tensors, build):
        def key():
            return tuple((t._version, t.data_ptr(), weight_epoch(t), tuple(t.shape)) for t in tensors)
        hit = self._c.get(role)
        if hit is not None and hit[0] == key():
            return hit[1]
        wp = build()
        self._c[role] = (key(), wp)              # taken after packing: pack mode 2 zeroes the masked taps of w in place
        return wp

    def get(self, w: torch.Tensor, role: int, masked: int = 0):
        pack = _PACKERS.get(role)
        return self._cached(role, (w,), lambda: pack(w) if pack is not None else F.pack_weight(w, role, masked))

    def get_c4gdn(self, w: torch.Tensor, gamma: torch.Tensor, K: int, R: int):
        """the combined (first-layer weight, GDN gamma) stream of F.conv2d_c4_gdn_f16x3, rebuilt when either parameter changed"""
        return self._cached(PACK_C4GDN, (w, gamma), lambda: F.c4gdn_stream(self.get(w, F.PACK_CONV_FWD_C4), gamma, K, R, R))


def _flat_grad(p):
    """The parameter's slot in a FlatParameters gradient buffer when `p.grad` currently IS that slot, else None.
    Weight / bias gradients are then accumulated straight into the slot by the unpack / column-sum kernels and the
    autograd Function returns None for them: exactly what AccumulateGrad's `p.grad += g` would do, without the
    temporary and the extra pass.  (Only `.backward()` accumulation is served this way; torch.autograd.grad() with
    these parameters as inputs would see None -- use plain parameters, i.e. no FlatParameters, for that.)"""
    view = getattr(p, "_flat_grad_view", None)
    return view if view is not None and p.grad is view else None


# Weight gradients are off the critical path of back-propagation (nothing downstream consumes them), so when they are
# accumulated straight into a flat gradient buffer they are launched on a side stream: the many small layers of the
# variable-rate models (16x16 .. 4x4 feature maps) then overlap their latency-bound wgrad / column-sum / unpack kernels
# with the dgrad chain.  All weight-gradient work shares that one stream (ordered among itself, so the shared
# geometry-keyed workspaces and repeated accumulation into one parameter stay race-free); the compute stream re-joins
# at the end of every backward pass (autograd engine callback) and wherever gradients are consumed (optim.py).
_WGRAD_SIDE = {"enabled": True, "streams": {}, "queued": False, "keep": []}


def wgrad_side_stream(device):
    st = _WGRAD_SIDE["streams"].get(device)
    if st is None:
        st = _WGRAD_SIDE["streams"][device] = F.make_stream(device, "side")
    return st


def join_wgrad_stream():
    """Order all outstanding side-stream weight-gradient work before whatever the current stream does next."""
    _WGRAD_SIDE["queued"] = False
    for dev, st in _WGRAD_SIDE["streams"].items():
        F.stream_wait(F.cur_stream(dev), st)
    _WGRAD_SIDE["keep"].clear()          # the current stream is now ordered after every reader (see _on_side_stream)


def _on_side_stream(fn, *tensors):
    dev = tensors[0].device
    side = wgrad_side_stream(dev)
    F.stream_wait(side, F.cur_stream(dev))
    with F.on_stream(side):
        fn()
    for t in tensors:
        t.record_stream(side)            # the allocator must not hand the memory out again before the side stream is done
    # ... and nobody may WRITE it before then either.  autograd sums fan-out gradients in place when it holds the last
    # reference to a buffer (InputBuffer::accumulate): the gradient of a residual add reaches a convolution's backward
    # AND, as the very same tensor, the skip connection, where the engine later does `dy.add_(dx_branch)` on the compute
    # stream -- while the weight-gradient kernel queued here may not have read dy yet.  (Observed as wrong conv_1
    # gradients of the residual blocks as soon as a second process competed for the GPU and delayed the side stream;
    # tests/test_hip_dp2.py.)  Holding a reference until the streams are joined keeps such buffers out of place.
    _WGRAD_SIDE["keep"].extend(tensors)
    if not _WGRAD_SIDE["queued"]:
        _WGRAD_SIDE["queued"] = True
        torch.autograd.Variable._execution_engine.queue_callback(join_wgrad_stream)


def _weight_grads(ctx, wgrad, *operands, flat=True):
    """(dw, db) of a convolution Function's backward.  `wgrad(gw, gb, need_db)` runs the kernels, accumulating into the tensors it
    is given or filling new ones (gw None), and returns them.  When the parameters' `.grad` are slots of a flat gradient buffer
    (_flat_grad) it accumulates straight into them on the side stream, `operands` (what it reads) held until the streams join."""
    if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
        return None, None
    need_db = bool(ctx.needs_input_grad[2])
    gw, gb = _flat_grad(ctx.params[0]), (_flat_grad(ctx.params[1]) if need_db else None)
    if not (flat and gw is not None and (gb is not None or not need_db)):
        return wgrad(None, None, need_db)

    def run():
        wgrad(gw, gb, need_db)
    _on_side_stream(run, *operands) if _WGRAD_SIDE["enabled"] else run()
    return None, None


# ----------------------------------------------------------------------------- which kernel serves a convolution
#: fewest output pixels for which the fp16 kernel beats the fp32-MFMA one (64-pixel tiles, no split-K: below ~3/4 of the CUs
#: the split-K fp32 kernel wins; measured on g_a.6 at B=16: 4096 pixels)
_F16X3_MIN_PIXELS = 12288
FP16 = ("wide", "gen")        # Route kinds of the split-operand fp16 kernels


def _planes_fit(npix, channels):
    """does a planes tensor of this size (4 bytes per element) stay inside one 2 GiB buffer view?"""
    return npix * ((channels + 31) // 32) * F.PLANES_SLAB_BYTES < 0x7FFFFF00


def f16x3_same_shape(stride, R, pad, C, K, k_multiple=32):
    """The shape rule of the stride-1 convolutions whose forward, input gradient and weight gradient run on the fp16 kernels
    (engine._Layer shares it): 'same' padding, an odd window of at most 25 taps, channel counts in whole 32-channel slabs.
    Odd windows only: with an even R the output is (H + 1) x (W + 1) and the input gradient needs pad R - 1 - pad, which the
    planes hand-over between layers ('same' shapes) does not carry."""
    return stride == 1 and R % 2 == 1 and R * R <= 25 and pad == R // 2 and C % 32 == 0 and K % k_multiple == 0


class Route(collections.namedtuple("Route", "kind gdn planes_out infer dgrad")):
    """Which kernels serve one convolution:
      kind        "c4"   the 4-channel-input fp32-MFMA kernel of igemm.hip (the image, or image + quality map);
                  "c4h"  first layer + GDN on the fp16 kernel of c4gdn_f16x3.hip
                  "wide" the 192-column fp16 kernel of conv_f16x3.hip (128-pixel workgroups, one weight stream per 128 pixels)
                  "gen"  the general fp16 kernel (64-pixel workgroups x 128-column tiles, split-K: built for the 16x16 latents)
                  "f32"  the fp32-MFMA kernels of igemm.hip / wgrad.hip
      gdn         the GDN / IGDN that follows runs in the same kernel
      planes_out  the output is written as fp16 planes for the next convolution (`infer`: INSTEAD of the fp32 tensor)
      infer       inference-only entry points (no autograd graph); otherwise the layer-wise autograd Functions, whose input
                  gradient runs on kernel family `dgrad`"""
    __slots__ = ()

    def __str__(self):
        return self.kind + ("+gdn" if self.gdn else "") + (" -> planes" if self.planes_out else "")


def _runtime(cfg):
    return cfg if cfg is not None else _config.runtime()


def _out_shape(m, in_shape):
    hw, R = in_shape[2:], m.kernel_size
    hw = F.deconv_out_hw(*hw, R, R, m.stride, m.padding, m.output_padding) if isinstance(m, ConvTranspose2d) else F.conv_out_hw(*hw, R, R, m.stride, m.padding)
    return (in_shape[0], m.out_channels) + tuple(hw)


def route(m, in_shape, src, *, grad, on_device, cfg=None, gdn=None, act=False, consumer=None, c4gdn=None):
    """The one decision of which kernel family serves convolution `m` (Conv2d / MaskedConv2d / ConvTranspose2d).  Pure: it reads
    the module's static facts and its arguments and touches no tensor.  in_shape: logical (B, C, H, W) of the input
      src        "nchw" | "nhwc": an fp32 tensor in that layout; "planes": fp16 planes alone (left by an `infer` producer)
      grad       autograd is on;  on_device: input and weights live on the GPU;  cfg: the runtime configuration (default: current)
      gdn        None | "gdn" | "igdn": what follows;  act: a (leaky) ReLU follows, folded into the layer-wise kernels' epilogue
      consumer   Route of the convolution that reads this one's output and could take planes from it, else None;  c4gdn: a
                 (K, R, S, inverse) -> bool in place of F.c4gdn_supported (the library's answer), for callers without the library"""
    cfg = _runtime(cfg)
    K, Cin, R = m.out_channels, m.in_channels, m.kernel_size
    npix = in_shape[0] * in_shape[2] * in_shape[3]
    hands = consumer is not None and consumer.kind in FP16 and K % 32 == 0

    def first_layer(inverse):
        return "c4h" if cfg.first_layer_f16x3 and (c4gdn or F.c4gdn_supported)(K, R, R, inverse) else "c4"
    if not grad and cfg.analysis_f16x3 and type(m) is Conv2d:
        # frozen / inference chain of convolutions (the analysis transform): operands pre-split into fp16 planes, the following
        # GDN fused, the output written as planes again when the next convolution takes them.  A chain starts where the next
        # convolution is eligible too -- either at the 3-channel first layer, whose kernel then writes planes, or with a split
        # pass over an fp32 tensor -- and runs until one is not eligible.
        chain = hands and consumer.infer
        if chain and gdn == "gdn" and Cin == 3 and src == "nchw" and K <= 192:
            return Route(first_layer(False), True, True, True, None)
        # the kernels address their operands through 2 GiB buffer views: a batch whose planes exceed one stays on the fp32 kernels
        fp16 = not m._masked and on_device and R * R <= 25 and Cin % 32 == 0 and _planes_fit(npix, Cin)
        nout = in_shape[0] * math.prod(_out_shape(m, in_shape)[2:])
        if fp16 and K <= 192 and _planes_fit(nout, K) and nout >= _F16X3_MIN_PIXELS and (src == "planes" or chain):
            return Route("wide", gdn == "gdn", chain, True, None)
        # small layers that end a planes chain (the last convolution of the analysis transform: 4096 output pixels at the bench
        # size) go to the general split-K kernel, which has no fused GDN
        if fp16 and src == "planes" and gdn is None and K % 4 == 0:
            return Route("gen", False, chain, True, None)
    if gdn is not None and not grad and K <= 192 and K % 4 == 0 and Cin % 4 in (0, 3):
        # Conv2d / ConvTranspose2d followed by GDN / IGDN in ONE kernel (inference only: no autograd graph)
        image = type(m) is not ConvTranspose2d and Cin == 3 and src == "nchw"
        return Route(first_layer(gdn == "igdn") if image else "f32", True, False, True, None)
    if isinstance(m, ConvTranspose2d):
        return Route("f32", False, False, False, "f32")
    # the layer-wise (autograd) Functions.  <= 4 input channels: the image (NCHW, fused layout change) or image + quality map
    if (Cin == 3 and src == "nchw") or (Cin == 4 and R * R <= 32):
        return Route("c4", False, False, False, "f32")
    # Stride-1 convolutions of the layer-wise models (the variable-rate family of models/stem_roi.py) on the fp16 matrix cores:
    # three fp16 products per fp32 product on two-plane operands, ~2^-21 per product (csrc/conv_f16x3.hip / wgrad_f16x3.hip);
    # STEM_LAYERS_F16X3=0: fp32 MFMA.  The general fp16 kernel streams its weight tile once per 64-pixel workgroup and the fp16
    # weight-gradient kernel re-reads both operands once per tap: at full-resolution feature maps (a million pixels per batch) both
    # are bound by L2 -> LDS traffic and lose to the 128x128-tile fp32-MFMA kernels: `layers_f16x3_maxpix` (sweep: DESIGN.md 9)
    if (on_device and cfg.layers_f16x3 and not m._masked and f16x3_same_shape(m.stride, R, m.padding, Cin, K)
            and npix <= cfg.layers_f16x3_maxpix and _planes_fit(npix, max(Cin, K)) and npix * ((max(K, Cin) + 127) // 128) * 512 < 0x7FFFFF00):
        def family(n_out):      # large pixel counts with at most 192 output channels: the 192-column kernel
            return "wide" if n_out <= 192 and npix >= cfg.layers_wide_minpix else "gen"
        # planes for the next convolution when both run on the fp16 kernels (a conv -> LeakyReLU -> conv chain)
        return Route(family(K), False, bool(act and hands and not consumer.infer), False, family(Cin))
    return Route("f32", False, False, False, "f32")


def planes_of(t):
    """the fp16 planes copy a producing kernel left next to an activation tensor (same values), if any.  An autograd Function
    returns tensors only: this attribute is how planes leave Conv2dFunction (_attach_planes) and reach the next convolution."""
    return getattr(t, "_stem_planes", None)


def _attach_planes(t, planes):
    if planes is not None:
        t._stem_planes = planes
    return t


def _src(x):
    return "nchw" if F.nhwc_ld(x) is None else "nhwc"


# ----------------------------------------------------------------------------- autograd functions
class Conv2dFunction(torch.autograd.Function):
    """Conv2d (+ leaky ReLU) on the layer-wise route `r`; `xp`: the input as planes where its producer left them"""

    @staticmethod
    def forward(ctx, x, weight, bias, r, xp, stride, pad, act, masked, cache, slope=F.LRELU_SLOPE):
        K, Cc, R, S = weight.shape
        yp = None
        if r.kind in FP16:
            # the input as planes (the producer's, or split here), kept for the weight gradient; the activation is the epilogue
            if xp is None or tuple(xp.shape) != tuple(x.shape):
                xp = F.F16Planes.split(x)
            if r.kind == "wide":
                y, yp = F.conv2d_f16x3_act(xp, cache.get(weight, PACK_F16X2), bias, K, R, S, 1, pad, bool(act), slope, r.planes_out)
            else:
                y, yp = F.conv2d_f16x3_gen(xp, cache.get(weight, PACK_F16X2_GEN), bias, K, R, S, 1, pad,
                                            epi=F.GEN_EPI_LRELU if act else F.GEN_EPI_BIAS, slope=slope, want_planes=r.planes_out)
            xin, ctx.planes = xp.data, (xp.q_offset, xp.pix_bytes, xp.byte_offset)
        elif r.kind == "c4":
            x4 = F.nchw3_to_nhwc4(x) if Cc == 3 else F.dense_nhwc(x).permute(0, 2, 3, 1)
            y = F.conv2d_fwd_c4(x4, cache.get(weight, F.PACK_CONV_FWD_C4), bias, K, R, S, stride, pad)
            if act:
                y = F.lrelu_fwd(y, slope)
            xin = x4.permute(0, 3, 1, 2)                # [B,4,H,W] NHWC view for the weight gradient
        else:
            xin = F.to_nhwc(x)
            y = F.conv2d_fwd(xin, cache.get(weight, F.PACK_CONV_FWD, masked), bias, K, R, S, stride, pad,
                             act | (F.CONV_MASKED_A if masked and not masked & 4 else 0), slope=slope)
        ctx.route, ctx.stride, ctx.pad, ctx.act, ctx.masked, ctx.cache, ctx.slope = r, stride, pad, act, masked, cache, slope
        ctx.xshape, ctx.params = tuple(x.shape), (weight, bias)
        ctx.save_for_backward(xin, weight, y if act else None)
        return _attach_planes(y, yp)

    @staticmethod
    def backward(ctx, dy):
        r, stride, pad, masked, cache, slope = ctx.route, ctx.stride, ctx.pad, ctx.masked, ctx.cache, ctx.slope
        xin, weight, y = ctx.saved_tensors
        K, Cc, R, S = weight.shape
        dy = F.to_nhwc(dy)
        if r.kind in FP16:
            xp = F.F16Planes(xin, ctx.xshape, *ctx.planes)
            # the gradient as planes, with this layer's leaky-ReLU derivative applied in the splitting pass
            dy = F.F16Planes.split_dact(dy, y, slope) if ctx.act else F.F16Planes.split(dy)
        else:
            if F.nhwc_ld(dy) != K:
                dy = F.copy_channels(dy, F.empty_nhwc(*dy.shape, dy.device))
            if ctx.act:
                dy = F.lrelu_bwd(y, dy, slope)
        dx = None
        if ctx.needs_input_grad[0] and r.dgrad == "wide":
            dx = F.conv2d_f16x3_act(dy, cache.get(weight, PACK_F16X2_FLIP), None, Cc, R, S, 1, pad)[0]
        elif ctx.needs_input_grad[0] and r.dgrad == "gen":
            dx = F.conv2d_f16x3_gen(dy, cache.get(weight, PACK_F16X2_GEN_FLIP), None, Cc, R, S, 1, pad, epi=F.GEN_EPI_BIAS)[0]
        elif ctx.needs_input_grad[0]:
            dx = F.conv2d_dgrad(dy, cache.get(weight, F.PACK_CONV_DGRAD, (1 | (masked & 4)) if masked else 0), ctx.xshape, K, R, S, stride, pad)
        if r.kind in FP16:
            def wgrad(gw, gb, need_db):
                if gw is None:
                    gw = torch.zeros((K, Cc, R, S), device=xin.device, dtype=torch.float32)
                    gb = torch.zeros(K, device=xin.device, dtype=torch.float32) if need_db else None
                F.conv2d_wgrad_f16x3_into(xp, dy, K, R, S, pad, gw, gb, accumulate=True)
                return gw, gb
            dw, db = _weight_grads(ctx, wgrad, dy.data, xin)
        else:
            def wgrad(gw, gb, need_db):
                return F.conv2d_wgrad(xin, dy, K, R, S, stride, pad, dw_out=gw, db_out=gb, need_db=need_db, accumulate=gw is not None)
            image = r.kind == "c4" and Cc == 3          # its weight gradient has the 4 channels of the padded image
            dw, db = _weight_grads(ctx, wgrad, dy, xin, flat=not image)
            if image and dw is not None:
                dw = dw[:, :3].contiguous()
        return dx, dw, db, None, None, None, None, None, None, None, None


class ConvTranspose2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, opad, act, cache, slope=F.LRELU_SLOPE):
        Cc, K, R, S = weight.shape
        xin = F.to_nhwc(x)
        y = F.deconv2d_fwd(xin, cache.get(weight, F.PACK_DECONV_FWD), bias, K, R, S, stride, pad, opad, act, slope=slope)
        ctx.stride, ctx.pad, ctx.opad, ctx.act, ctx.cache, ctx.slope = stride, pad, opad, act, cache, slope
        ctx.xshape, ctx.params = tuple(x.shape), (weight, bias)
        ctx.save_for_backward(xin, weight, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        stride, pad, opad, act, cache = ctx.stride, ctx.pad, ctx.opad, ctx.act, ctx.cache
        xin, weight, y = ctx.saved_tensors
        Cc, K, R, S = weight.shape
        dy = F.to_nhwc(dy)
        # The synthesis transform's last layer (-> 3 image channels): the image gradient is padded to 4 channels so that
        # the input gradient is the 4-channel-input convolution kernel (it IS Conv2d(weight [C,3,R,S], stride, pad) applied
        # to dY) and the weight gradient uses the folded-tap mode, instead of 3-wide operands in 64-wide MFMA tiles.
        rgb = K == 3 and not act and R * S <= 32
        if rgb:
            B, _, Ho, Wo = dy.shape
            dy4 = torch.zeros((B, Ho, Wo, 4), device=dy.device, dtype=torch.float32)
            F.copy_channels(dy, dy4.permute(0, 3, 1, 2)[:, :3])
            dy = dy4.permute(0, 3, 1, 2)
        else:
            if F.nhwc_ld(dy) != K:
                dy = F.copy_channels(dy, F.empty_nhwc(*dy.shape, dy.device))
            if act:
                dy = F.lrelu_bwd(y, dy, ctx.slope)
        dx = None
        if ctx.needs_input_grad[0] and rgb:
            dx = F.conv2d_fwd_c4(dy4, cache.get(weight, F.PACK_CONV_FWD_C4), None, Cc, R, S, stride, pad)
            assert tuple(dx.shape) == tuple(ctx.xshape), (dx.shape, ctx.xshape)
        elif ctx.needs_input_grad[0]:
            dx = F.deconv2d_dgrad(dy, cache.get(weight, F.PACK_DECONV_DGRAD), ctx.xshape, K, R, S, stride, pad, opad)

        def wgrad(gw, gb, need_db):
            return F.deconv2d_wgrad(xin, dy, 4 if rgb else K, R, S, stride, pad, opad, dw_out=gw, db_out=gb, need_db=need_db,
                                    accumulate=gw is not None)
        dw, db = _weight_grads(ctx, wgrad, dy, xin, flat=not rgb)
        if rgb and dw is not None:
            dw, db = dw[:, :3].contiguous(), (db[:3].contiguous() if db is not None else None)
        return dx, dw, db, None, None, None, None, None, None


class GDNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, beta, gamma, inverse, beta_min):
        xin = F.to_nhwc(x)
        ctx.cfg = (inverse, beta_min)
        ctx.save_for_backward(xin, beta, gamma)
        return F.gdn_fwd(xin, beta, gamma, inverse, beta_min)

    @staticmethod
    def backward(ctx, dy):
        inverse, beta_min = ctx.cfg
        xin, beta, gamma = ctx.saved_tensors
        dy = F.to_nhwc(dy)
        if F.nhwc_ld(dy) % 4 or F.nhwc_ld(xin) % 4:
            raise NotImplementedError("GDN backward needs channel counts that are multiples of 4")
        dx, dbeta, dgamma = F.gdn_bwd(xin, dy, beta.detach().contiguous(), gamma.detach().contiguous(), inverse, beta_min)
        return dx, dbeta, dgamma, None, None


class GDN1Function(torch.autograd.Function):
    """GDN1 on the kernels of csrc/gdn1.hip: any channel count up to F.GDN1_MAX_C; the backward computes what is asked for"""

    @staticmethod
    def forward(ctx, x, beta, gamma, inverse, beta_min):
        xin = F.to_nhwc(x)
        ctx.cfg = (inverse, beta_min)
        ctx.save_for_backward(xin, beta, gamma)
        return F.gdn1_forward(xin, beta, gamma, inverse, beta_min)

    @staticmethod
    def backward(ctx, dy):
        inverse, beta_min = ctx.cfg
        xin, beta, gamma = ctx.saved_tensors
        need_dx, need_dparams = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (need_dx or need_dparams):
            return None, None, None, None, None
        dx, dbeta, dgamma = F.gdn1_backward(xin, F.to_nhwc(dy), beta, gamma, inverse, beta_min, need_dx, need_dparams)
        return dx, (dbeta if ctx.needs_input_grad[1] else None), (dgamma if ctx.needs_input_grad[2] else None), None, None


class SFTFunction(torch.autograd.Function):
    """act(x * (1 + gamma) + beta), act = leaky-ReLU(slope) or identity (slope 1): stem_utils.py:41,56-57."""

    @staticmethod
    def forward(ctx, x, gamma, beta, slope):
        x, gamma, beta = (F.dense_nhwc(t) for t in (x, gamma, beta))
        out = F.sft_fwd(x, gamma, beta, slope)
        ctx.slope = slope
        ctx.save_for_backward(x, gamma, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, gamma, out = ctx.saved_tensors
        dx, dg, db = F.sft_bwd(x, gamma, out, F.dense_nhwc(dout), ctx.slope)
        return dx, dg, db, None


class AvgPoolFunction(torch.autograd.Function):
    """F.adaptive_avg_pool2d(x, (Ho, Wo)) for integer ratios (stem_utils.py:37, stem_roi.py:563)."""

    @staticmethod
    def forward(ctx, x, Ho, Wo):
        ctx.hw = tuple(x.shape[2:])
        return F.avgpool(F.to_nhwc(x), Ho, Wo)

    @staticmethod
    def backward(ctx, dy):
        return F.avgpool_bwd(F.to_nhwc(dy), *ctx.hw), None, None


class CatFunction(torch.autograd.Function):
    """torch.cat(xs, dim=1) into one NHWC buffer; the gradient hands back channel-slice views."""

    @staticmethod
    def forward(ctx, *xs):
        B, _, H, W = xs[0].shape
        ctx.widths = [int(t.shape[1]) for t in xs]
        buf = F.empty_nhwc(B, sum(ctx.widths), H, W, xs[0].device)
        c = 0
        for t, n in zip(xs, ctx.widths):
            F.copy_channels(F.to_nhwc(t), buf[:, c:c + n])
            c += n
        return buf

    @staticmethod
    def backward(ctx, dy):
        dy = F.to_nhwc(dy)
        outs, c = [], 0
        for n in ctx.widths:
            outs.append(dy[:, c:c + n])
            c += n
        return tuple(outs)


class AddFunction(torch.autograd.Function):
    """Residual sum x + dx (stem_utils.py:58) on dense NHWC tensors."""

    @staticmethod
    def forward(ctx, a, b):
        return F.add(F.dense_nhwc(a), F.dense_nhwc(b))

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


class PixelShuffleFunction(torch.autograd.Function):
    """act(PixelShuffle(r)(x)) (+ addend) in one pass: the sub-pixel convolutions of compressai/layers/layers.py:55-59 with the
    leaky ReLU / `out += identity` that follow them in ResidualBlockUpsample (layers.py:118-126); slope 1.0: no activation."""

    @staticmethod
    def forward(ctx, x, r, slope, addend):
        xin = F.to_nhwc(x)
        ctx.r, ctx.slope = int(r), float(slope)
        ctx.save_for_backward(xin if ctx.slope != 1.0 else None)
        return F.pixel_shuffle(xin, ctx.r, ctx.slope, None if addend is None else F.to_nhwc(addend))

    @staticmethod
    def backward(ctx, dout):
        (xin,) = ctx.saved_tensors
        dout = F.to_nhwc(dout)
        dx = F.pixel_shuffle_backward(dout, ctx.r, xin, ctx.slope) if ctx.needs_input_grad[0] else None
        return dx, None, None, (dout if ctx.needs_input_grad[3] else None)


class AddActFunction(torch.autograd.Function):
    """act(a + b), act = LeakyReLU(slope), slope 0 = ReLU: ResidualUnit's relu(conv(x) + x) (compressai/layers/layers.py:191-196)"""

    @staticmethod
    def forward(ctx, a, b, slope):
        out = F.add_act(F.to_nhwc(a), F.to_nhwc(b), float(slope))
        ctx.slope = float(slope)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        g = F.add_act_backward(out, F.to_nhwc(dout), ctx.slope)
        return g, g, None


class GateFunction(torch.autograd.Function):
    """a * sigmoid(b) + x: AttentionBlock.forward (compressai/layers/layers.py:207-213); the sigmoid is recomputed in the backward pass"""

    @staticmethod
    def forward(ctx, a, b, x):
        a, b = F.to_nhwc(a), F.to_nhwc(b)
        ctx.save_for_backward(a, b)
        return F.gate(a, b, F.to_nhwc(x))

    @staticmethod
    def backward(ctx, dout):
        a, b = ctx.saved_tensors
        dout = F.to_nhwc(dout)
        da, db = F.gate_backward(a, b, dout)
        return da, db, dout


class AbsFunction(torch.autograd.Function):
    """torch.abs on NHWC memory: the |y| in front of ScaleHyperprior's h_a (compressai/models/priors.py:258)"""

    @staticmethod
    def forward(ctx, x):
        xin = F.to_nhwc(x)
        ctx.save_for_backward(xin)
        return F.abs_(xin)

    @staticmethod
    def backward(ctx, g):
        (xin,) = ctx.saved_tensors
        return F.abs_backward(xin, F.to_nhwc(g))


class ToNCHWFunction(torch.autograd.Function):
    """NHWC feature map -> contiguous NCHW tensor (the image handed back to the caller)."""

    @staticmethod
    def forward(ctx, x):
        return F.to_nchw(F.to_nhwc(x))

    @staticmethod
    def backward(ctx, dy):
        return F.to_nhwc(dy)


def cat(xs):
    return CatFunction.apply(*xs)


def to_nchw(x):
    return ToNCHWFunction.apply(x)


def adaptive_avg_pool2d(x, size):
    if tuple(x.shape[2:]) == tuple(size):
        return x
    return AvgPoolFunction.apply(x, int(size[0]), int(size[1]))


# ----------------------------------------------------------------------------- modules
def _pair(v):
    return v if isinstance(v, int) else v[0]


class Conv2d(nn.Module):
    """nn.Conv2d(in, out, kernel_size, stride, padding) with square kernels, bias, dilation 1."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride, self.padding = _pair(kernel_size), _pair(stride), _pair(padding)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, self.kernel_size, self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self._packs = _PackCache()
        self._masked = 0
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))      # nn.Conv2d default; models re-init (priors.py:67-72)
        if self.bias is not None:
            bound = 1 / math.sqrt(self.weight[0].numel())
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x, act=F.ACT_NONE, slope=F.LRELU_SLOPE, r=None):
        """r: the layer-wise Route a FusedSequential has planned for this call"""
        r = r or route(self, x.shape, _src(x), grad=torch.is_grad_enabled(), on_device=x.is_cuda)
        return Conv2dFunction.apply(x, self.weight, self.bias, r, planes_of(x), self.stride, self.padding, act, self._masked, self._packs, slope)

    def _launch(self, r, x, xp, gdn, act, slope):
        """the kernels of route `r` on (fp32 tensor or None, planes or None) -> the same pair for the next step"""
        K, R, w, b, packs = self.out_channels, self.kernel_size, self.weight, self.bias, self._packs
        if not r.infer:
            y = self(x, act, slope, r)
            return y, planes_of(y)
        beta, gamma, beta_min = (gdn.beta, gdn.gamma, gdn.beta_min) if r.gdn else (None, None, 1e-6)
        if r.kind in ("c4", "c4h"):
            wp = packs.get(w, F.PACK_CONV_FWD_C4) if r.planes_out else None
            ast = packs.get_c4gdn(w, gamma, K, R) if r.kind == "c4h" else None
            x4 = F.nchw3_to_nhwc4(x)
            if r.planes_out:
                return None, F.conv2d_fwd_c4_gdn_planes(x4, wp, b, beta, gamma, K, R, R, self.stride, self.padding, beta_min, astream=ast)
            return F.conv2d_fwd_c4_gdn(x4, packs.get(w, F.PACK_CONV_FWD_C4), b, beta, gamma, K, R, R, self.stride, self.padding,
                                       gdn.inverse, beta_min, astream=ast), None
        if r.kind == "wide":
            xin = xp if x is None else F.F16Planes.split(x)
            wp = packs.get(w, PACK_F16X2)
            gp = packs.get(gamma, PACK_GDN_GAMMA) if r.gdn else None          # kept in the convolution's cache
            out = F.conv2d_f16x3_fwd(xin, wp, b, K, R, R, self.stride, self.padding, beta, gamma, beta_min, planes_out=r.planes_out, gp=gp)
            return (None, out) if r.planes_out else (out, None)
        if r.kind == "gen":
            return F.conv2d_f16x3_gen(xp, packs.get(w, PACK_F16X2_GEN), b, K, R, R, self.stride, self.padding,
                                      want_fp32=not r.planes_out, want_planes=r.planes_out)
        return F.conv2d_gdn_fwd(F.to_nhwc(x), packs.get(w, F.PACK_CONV_FWD, self._masked), b, beta, gamma, K, R, R, self.stride,
                                self.padding, gdn.inverse, beta_min), None

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}"


class ConvTranspose2d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, output_padding=0, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride, self.padding = _pair(kernel_size), _pair(stride), _pair(padding)
        self.output_padding = _pair(output_padding)
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, self.kernel_size, self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self._packs = _PackCache()
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.weight.shape[0] * self.kernel_size ** 2)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x, act=F.ACT_NONE, slope=F.LRELU_SLOPE):
        return ConvTranspose2dFunction.apply(x, self.weight, self.bias, self.stride, self.padding, self.output_padding,
                                             act, self._packs, slope)

    def _launch(self, r, x, xp, gdn, act, slope):
        if not r.gdn:
            return self(x, act, slope), None
        R = self.kernel_size
        return F.deconv2d_gdn_fwd(F.to_nhwc(x), self._packs.get(self.weight, F.PACK_DECONV_FWD), self.bias, gdn.beta, gdn.gamma,
                                  self.out_channels, R, R, self.stride, self.padding, self.output_padding, gdn.inverse, gdn.beta_min), None


class MaskedConv2d(Conv2d):
    """PixelCNN-style masked convolution; like the reference the masked taps of `weight` are zeroed
    *in place* at every forward (the pack kernel does it) while their gradients stay unmasked."""

    def __init__(self, *args, mask_type="A", **kwargs):
        super().__init__(*args, **kwargs)
        if mask_type not in ("A", "B"):
            raise ValueError(f'Invalid "mask_type" value "{mask_type}"')
        self.register_buffer("mask", torch.ones_like(self.weight.data))
        _, _, h, w = self.mask.size()
        self.mask[:, :, h // 2, w // 2 + (mask_type == "B"):] = 0
        self.mask[:, :, h // 2 + 1:] = 0
        # pack-kernel mode 2 (zero the masked taps of `weight` in place, as the reference's forward does) | 4 for type B.
        # Type A (the STEM context model, spatiotemporalpriors.py:546,830) additionally lets the kernel skip the dead taps.
        self._masked = 2 | (4 if mask_type == "B" else 0)


class GDN(nn.Module):
    def __init__(self, in_channels, inverse=False, beta_min=1e-6, gamma_init=0.1):
        super().__init__()
        self.inverse = bool(inverse)
        self.beta_min = float(beta_min)
        self.beta_reparam = NonNegativeParametrizer(minimum=beta_min)
        self.beta = nn.Parameter(self.beta_reparam.init(torch.ones(in_channels)))
        self.gamma_reparam = NonNegativeParametrizer()
        self.gamma = nn.Parameter(self.gamma_reparam.init(float(gamma_init) * torch.eye(in_channels)))

    def forward(self, x):
        return GDNFunction.apply(x, self.beta, self.gamma, self.inverse, self.beta_min)


class GDN1(GDN):
    """Simplified GDN (compressai/layers/gdn.py:70-96): y = x / (beta + gamma |x|), no square and no square root.  A GDN by class,
    as in the reference, with the same parameters and state-dict keys -- but never by kernel: FusedSequential runs it as a step of
    its own, so it cannot reach the squared GDN fused into the convolution kernels."""

    def forward(self, x):
        return GDN1Function.apply(x, self.beta, self.gamma, self.inverse, self.beta_min)


def _fusable_gdn(m):
    """a GDN the conv+GDN kernels compute: the squared form only"""
    return isinstance(m, GDN) and not isinstance(m, GDN1)


class LeakyReLU(nn.LeakyReLU):
    """Placeholder that keeps nn.Sequential indices (`HE.0`, `HE.2`, …) identical to the reference;
    FusedSequential folds it into the preceding convolution's epilogue."""


#: One step of a plan: the children it covers (conv [+ GDN | + activation]; a lone GDN / activation: route None), the input's shape
Step = collections.namedtuple("Step", "children route in_shape act slope")
_ACTIVATIONS = (nn.LeakyReLU, nn.ReLU)


class FusedSequential(nn.Sequential):
    #: optional (index, list) pair -- or a dict {index: list} -- set by bench.py: HIP events are recorded on the launching stream
    #: around the kernel(s) of the step whose first child is `index`
    probe = None

    def _timed(self, i, fn):
        probe = self.probe
        sink = probe.get(i) if isinstance(probe, dict) else probe[1] if probe is not None and probe[0] == i else None
        if sink is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        sink.append((e0, e1))
        return out

    def plan(self, in_shape, src, grad, on_device, cfg=None, c4gdn=None):
        """The children as a list of Steps for an input of logical shape `in_shape` (other arguments: see `route`).  Pure and cheap:
        planned at every call.  A GDN behind a convolution is fused where the route has a kernel for it (a GDN1 never is: always a
        lone step); a LeakyReLU (slope) or ReLU (= slope 0) is folded into the layer-wise kernels' epilogue; planes travel between
        convolutions on the fp16 kernels."""
        mods, steps, shape, i = list(self), [], tuple(in_shape), 0
        kw = dict(grad=grad, on_device=on_device, cfg=_runtime(cfg), c4gdn=c4gdn)

        def routed(j, shape, src, consumer=None):
            nxt = mods[j + 1] if j + 1 < len(mods) else None
            gdn = ("igdn" if nxt.inverse else "gdn") if _fusable_gdn(nxt) else None
            return route(mods[j], shape, src, gdn=gdn, act=isinstance(nxt, _ACTIVATIONS), consumer=consumer, **kw)

        while i < len(mods):
            m = mods[i]
            if isinstance(m, (GDN,) + _ACTIVATIONS):
                steps.append(Step((i,), None, shape, F.ACT_NONE, F.LRELU_SLOPE))
                src, i = "nhwc" if isinstance(m, GDN) else src, i + 1
                continue
            if not isinstance(m, (Conv2d, ConvTranspose2d)):
                raise TypeError(f"FusedSequential plans convolutions, GDNs and (leaky) ReLUs; child {i} is a {type(m).__name__}")
            # who reads the output: the convolution behind a fusable GDN / a folded activation, or the very next child
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            folded = isinstance(nxt, _ACTIVATIONS)
            j = i + (2 if folded or (_fusable_gdn(nxt) and not nxt.inverse) else 1)
            out_shape, consumer = _out_shape(m, shape), None
            if j < len(mods) and type(mods[j]) is Conv2d and mods[j].in_channels == m.out_channels:
                consumer = routed(j, out_shape, "nhwc" if folded else "planes")
            r = routed(i, shape, src, consumer)
            assert src != "planes" or (r.infer and r.kind in FP16), f"child {i} was handed planes and has no kernel that reads them ({r})"
            act, slope = F.ACT_NONE, F.LRELU_SLOPE
            if folded and not r.infer:
                act, slope = F.ACT_LRELU, (float(nxt.negative_slope) if isinstance(nxt, nn.LeakyReLU) else 0.0)
            n = 2 if r.gdn or act else 1
            steps.append(Step(tuple(range(i, i + n)), r, shape, act, slope))
            shape, src, i = out_shape, "planes" if r.infer and r.planes_out else "nhwc", i + n
        return steps

    def forward(self, x):
        mods, xp = list(self), planes_of(x)
        for st in self.plan(x.shape, _src(x), torch.is_grad_enabled(), x.is_cuda):
            m = mods[st.children[0]]
            if st.route is None:
                x, xp = m(x), None
                continue
            gdn = mods[st.children[1]] if st.route.gdn else None
            x, xp = self._timed(st.children[0], lambda: m._launch(st.route, x, xp, gdn, st.act, st.slope))
        return x


def conv(in_channels, out_channels, kernel_size=5, stride=2):
    """compressai/models/utils.py:112-120"""
    return Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=kernel_size // 2)


def deconv(in_channels, out_channels, kernel_size=5, stride=2):
    """compressai/models/utils.py:122-130"""
    return ConvTranspose2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride,
                           output_padding=stride - 1, padding=kernel_size // 2)


# the residual / sub-pixel / attention blocks of the cheng2020 models, built on the pieces above
from .layers_residual import *  # noqa: E402,F401,F403
