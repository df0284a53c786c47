"""The building blocks of the cheng2020 I-frame models (compressai/layers/layers.py:50-213) on NHWC tensors: small convolutions
on the routes of `layers.route`, and the three fused device passes of csrc/resblock.hip between them.

  conv3x3 / conv1x1 / subpel_conv3x3 / PixelShuffle
  ResidualBlock, ResidualBlockWithStride, ResidualBlockUpsample, AttentionBlock
  BlockSequential      nn.Sequential over convolutions, sub-pixel convolutions, LeakyReLUs and blocks

Attribute names, and with them the state-dict keys, are the reference's; parameter-free members (`leaky_relu`, `relu`) are kept
because they carry the slopes.  Every block takes an NCHW or NHWC tensor and returns NHWC memory.  What is fused:
  conv -> LeakyReLU / ReLU            the convolution's epilogue (`act=`)
  conv -> GDN / IGDN                  one kernel under no_grad where `route(..., gdn=...)` has one; GDNFunction otherwise
  PixelShuffle -> LeakyReLU           the shuffle pass applies it
  PixelShuffle, `out += identity`     the shuffle of the identity branch adds `out` while it writes (ResidualBlockUpsample)
  relu(conv(x) + x)                   one pass (AddActFunction);  a * sigmoid(b) + x: one pass (GateFunction)
"""
import torch
import torch.nn as nn

from . import functional as F
from . import layers as L

__all__ = ["conv3x3", "conv1x1", "subpel_conv3x3", "PixelShuffle", "ResidualBlock", "ResidualBlockWithStride", "ResidualBlockUpsample",
           "AttentionBlock", "BlockSequential"]


def conv3x3(in_ch, out_ch, stride=1):
    """3x3 convolution with padding 1 (layers.py:50-52)"""
    return L.Conv2d(in_ch, out_ch, kernel_size=3, stride=stride, padding=1)


def conv1x1(in_ch, out_ch, stride=1):
    """1x1 convolution (layers.py:62-64)"""
    return L.Conv2d(in_ch, out_ch, kernel_size=1, stride=stride)


class PixelShuffle(nn.Module):
    """nn.PixelShuffle(upscale_factor) on NHWC memory; `slope` / `addend`: the fused forms the blocks use"""

    def __init__(self, upscale_factor):
        super().__init__()
        self.upscale_factor = int(upscale_factor)

    def forward(self, x, slope=1.0, addend=None):
        return L.PixelShuffleFunction.apply(x, self.upscale_factor, slope, addend)

    def extra_repr(self):
        return f"upscale_factor={self.upscale_factor}"


def subpel_conv3x3(in_ch, out_ch, r=1):
    """3x3 sub-pixel convolution for up-sampling (layers.py:55-59): keys `0.weight`, `0.bias`"""
    return nn.Sequential(L.Conv2d(in_ch, out_ch * r ** 2, kernel_size=3, padding=1), PixelShuffle(r))


def _subpel(seq, x, slope=1.0, addend=None):
    return seq[1](seq[0](x), slope, addend)


def _conv(m, x, slope=None, gdn=None):
    """convolution `m`, then a leaky ReLU of `slope` (None: none) or the GDN module `gdn`, on the route `layers.route` gives"""
    if gdn is not None and not L._fusable_gdn(gdn):          # a GDN1: never inside a convolution's kernel
        return gdn(_conv(m, x, slope))
    act = F.ACT_NONE if slope is None else F.ACT_LRELU
    slope = F.LRELU_SLOPE if slope is None else float(slope)
    r = L.route(m, x.shape, L._src(x), grad=torch.is_grad_enabled(), on_device=x.is_cuda,
                gdn=None if gdn is None else ("igdn" if gdn.inverse else "gdn"), act=bool(act))
    if r.infer:
        return m._launch(r, x, None, gdn, act, slope)[0]
    y = m(x, act, slope, r)
    return y if gdn is None else gdn(y)


def _slope(act):
    return float(act.negative_slope) if isinstance(act, nn.LeakyReLU) else 0.0


class ResidualBlockWithStride(nn.Module):
    """layers.py:67-98: conv3x3(stride) -> leaky ReLU -> conv3x3 -> GDN, plus the input (through a strided 1x1 where shapes differ)"""

    def __init__(self, in_ch, out_ch, stride=2):
        super().__init__()
        self.conv1 = conv3x3(in_ch, out_ch, stride=stride)
        self.leaky_relu = L.LeakyReLU(inplace=True)
        self.conv2 = conv3x3(out_ch, out_ch)
        self.gdn = L.GDN(out_ch)
        self.skip = conv1x1(in_ch, out_ch, stride=stride) if stride != 1 or in_ch != out_ch else None

    def forward(self, x):
        out = _conv(self.conv1, x, _slope(self.leaky_relu))
        out = _conv(self.conv2, out, gdn=self.gdn)
        return L.AddFunction.apply(out, x if self.skip is None else _conv(self.skip, x))


class ResidualBlockUpsample(nn.Module):
    """layers.py:101-126: subpel_conv3x3 -> leaky ReLU -> conv3x3 -> IGDN, plus a second sub-pixel convolution of the input"""

    def __init__(self, in_ch, out_ch, upsample=2):
        super().__init__()
        self.subpel_conv = subpel_conv3x3(in_ch, out_ch, upsample)
        self.leaky_relu = L.LeakyReLU(inplace=True)
        self.conv = conv3x3(out_ch, out_ch)
        self.igdn = L.GDN(out_ch, inverse=True)
        self.upsample = subpel_conv3x3(in_ch, out_ch, upsample)

    def forward(self, x):
        out = _subpel(self.subpel_conv, x, _slope(self.leaky_relu))
        out = _conv(self.conv, out, gdn=self.igdn)
        return _subpel(self.upsample, x, addend=out)


class ResidualBlock(nn.Module):
    """layers.py:129-159: two 3x3 convolutions with leaky ReLUs, plus the input (through a 1x1 where the widths differ)"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv1 = conv3x3(in_ch, out_ch)
        self.leaky_relu = L.LeakyReLU(inplace=True)
        self.conv2 = conv3x3(out_ch, out_ch)
        self.skip = conv1x1(in_ch, out_ch) if in_ch != out_ch else None

    def forward(self, x):
        slope = _slope(self.leaky_relu)
        out = _conv(self.conv2, _conv(self.conv1, x, slope), slope)
        return L.AddFunction.apply(out, x if self.skip is None else _conv(self.skip, x))


class _ResidualUnit(nn.Module):
    """layers.py:177-196: relu(conv1x1 -> ReLU -> conv3x3 -> ReLU -> conv1x1 of x, + x), at half the width inside"""

    def __init__(self, N):
        super().__init__()
        self.conv = L.FusedSequential(conv1x1(N, N // 2), nn.ReLU(inplace=True), conv3x3(N // 2, N // 2), nn.ReLU(inplace=True),
                                      conv1x1(N // 2, N))
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return L.AddActFunction.apply(self.conv(x), x, _slope(self.relu))


class AttentionBlock(nn.Module):
    """layers.py:162-213: a * sigmoid(b) + x with a, b two stacks of residual units over x (b ends in a 1x1)"""

    def __init__(self, N):
        super().__init__()
        self.conv_a = nn.Sequential(_ResidualUnit(N), _ResidualUnit(N), _ResidualUnit(N))
        self.conv_b = nn.Sequential(_ResidualUnit(N), _ResidualUnit(N), _ResidualUnit(N), conv1x1(N, N))

    def forward(self, x):
        return L.GateFunction.apply(self.conv_a(x), self.conv_b(x), x)


class BlockSequential(nn.Sequential):
    """nn.Sequential over what the cheng2020 transforms are made of.  A LeakyReLU behind a convolution runs in that convolution's
    epilogue, one behind a sub-pixel convolution in the shuffle pass; blocks are called as they are."""

    def forward(self, x):
        mods, i = list(self), 0
        while i < len(mods):
            m, nxt = mods[i], mods[i + 1] if i + 1 < len(mods) else None
            slope = _slope(nxt) if isinstance(nxt, nn.LeakyReLU) else None
            if isinstance(m, L.Conv2d):
                x = _conv(m, x, slope)
            elif isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[0], L.Conv2d) and isinstance(m[1], PixelShuffle):
                x = _subpel(m, x, 1.0 if slope is None else slope)
            elif slope is None and not isinstance(m, nn.LeakyReLU):
                x = m(x)
            else:
                raise TypeError(f"BlockSequential folds a LeakyReLU into the convolution or sub-pixel convolution in front of it; "
                                f"child {i} is a {type(m).__name__}")
            i += 1 if slope is None else 2
        return x
