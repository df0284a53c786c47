"""Colour transforms between RGB and YCbCr 4:4:4 / 4:2:0 tensors in [0,1] (ITU-R BT.709, full range): the surface of the reference's
compressai/transforms (functional.py:26-135, transforms.py:11-117) -- same names, arguments, modes and error types.

    rgb2ycbcr(rgb)                  ycbcr2rgb(ycbcr)                       3-D [3,H,W] or 4-D [N,3,H,W] floating-point tensors
    yuv_444_to_420(yuv, mode)       yuv_420_to_444(yuv, mode, return_tuple)   4-D tensors / tuples of three [N,1,H,W] planes
    RGB2YCbCr, YCbCr2RGB, YUV444To420, YUV420To444                          the callables a transform pipeline composes

Host tensors are computed with torch, in the reference's order of operations (bit-identical results: tests/test_yuv_abi.py), so
the module works inside a data-loader worker.  fp32 device tensors go to HIP kernels (csrc/yuv.hip), never to eager torch:

    rgb2ycbcr, ycbcr2rgb                    stem_ycbcr_convert     element-wise, fp32, the same order of operations
    yuv_444_to_420, yuv_420_to_444          stem_plane_resample2   one launch per chroma plane (2 x 2 mean; bilinear / nearest x2)
    yuv420_planes_to_rgb(planes)            stem_yuv420_to_rgb     = ycbcr2rgb(yuv_420_to_444(planes / peak, mode)) on INTEGER planes
    rgb_to_yuv420_planes(rgb)               stem_rgb_to_yuv420     = yuv_444_to_420(rgb2ycbcr(rgb)) [quantised]

The last two are the fused forms a sequence reader or writer uses (data.YUVSequence, data.write_yuv420).

Two deliberate differences from the reference.  Its YUV420To444.__call__ forgets its `mode` (transforms.py:115 passes return_tuple
only, so "nearest" is silently bilinear); here the mode given to the constructor is the mode used.  And its yuv_420_to_444(mode=
"nearest") hands align_corners=False to F.interpolate, which torch refuses for that mode, so it raises; here "nearest" works.
"""
from __future__ import annotations

import torch
import torch.nn.functional as tnf
from torch import Tensor

__all__ = ["rgb2ycbcr", "ycbcr2rgb", "yuv_444_to_420", "yuv_420_to_444", "RGB2YCbCr", "YCbCr2RGB", "YUV444To420", "YUV420To444",
           "yuv420_planes_to_rgb", "rgb_to_yuv420_planes"]

# luma weights of red, green and blue (ITU-R BT.709); the three sum to one
LUMA_R, LUMA_G, LUMA_B = 0.2126, 0.7152, 0.0722
UPSAMPLING, DOWNSAMPLING = ("bilinear", "nearest"), ("avg_pool",)
_RESAMPLE_MODE = {"bilinear": 0, "nearest": 1, "avg_pool": 2}          # stem_plane_resample2


def _image_channels(t, what="input"):
    """the three channel planes of a floating-point [3,H,W] / [N,3,H,W] tensor (channel axis kept), or the reference's ValueError"""
    ok = isinstance(t, Tensor) and t.is_floating_point() and t.dim() in (3, 4) and t.shape[-3] == 3
    if not ok:
        raise ValueError(f"Expected a 3D or 4D tensor with shape (Nx3xHxW) or (3xHxW) as {what}")
    return tuple(t.narrow(-3, k, 1) for k in range(3))


def _device_convert(t, to_rgb):
    from . import functional
    return functional.ycbcr_convert(t, to_rgb)


def _device_resample(plane, mode):
    """[N,1,H,W] device plane -> resampled [N,1,H',W'] by stem_plane_resample2"""
    from . import functional
    n, c, h, w = plane.shape
    out = functional.plane_resample2(plane.reshape(n * c, h, w), _RESAMPLE_MODE[mode])
    return out.view(n, c, *out.shape[-2:])


def _chroma_of(colour, luma, weight):
    """Cb (from blue) or Cr (from red): the colour difference scaled into [0,1] around 0.5"""
    return 0.5 * (colour - luma) / (1 - weight) + 0.5


def _colour_of(luma, chroma, weight):
    """blue (from Cb) or red (from Cr): the inverse of `_chroma_of`"""
    return luma + (2 - 2 * weight) * (chroma - 0.5)


def rgb2ycbcr(rgb: Tensor) -> Tensor:
    """RGB -> YCbCr, BT.709: Y is the weighted sum of r, g, b; Cb and Cr the blue and red differences from it"""
    red, green, blue = _image_channels(rgb)
    if rgb.is_cuda:
        return _device_convert(rgb, to_rgb=False)
    luma = LUMA_R * red + LUMA_G * green + LUMA_B * blue
    return torch.cat((luma, _chroma_of(blue, luma, LUMA_B), _chroma_of(red, luma, LUMA_R)), dim=-3)


def ycbcr2rgb(ycbcr: Tensor) -> Tensor:
    """YCbCr -> RGB, BT.709: red and blue from Y and their chroma, green from what Y leaves after them"""
    luma, cb, cr = _image_channels(ycbcr)
    if ycbcr.is_cuda:
        return _device_convert(ycbcr, to_rgb=True)
    red, blue = _colour_of(luma, cr, LUMA_R), _colour_of(luma, cb, LUMA_B)
    green = (luma - LUMA_R * red - LUMA_B * blue) / LUMA_G
    return torch.cat((red, green, blue), dim=-3)


def _resample(plane, mode):
    """one chroma plane [N,1,H,W] to half (DOWNSAMPLING modes) or twice (UPSAMPLING modes) its size"""
    if plane.is_cuda:
        return _device_resample(plane, mode)
    if mode == "avg_pool":
        return tnf.avg_pool2d(plane, kernel_size=2, stride=2)
    if mode == "bilinear":
        return tnf.interpolate(plane, scale_factor=2, mode="bilinear", align_corners=False)
    return tnf.interpolate(plane, scale_factor=2, mode="nearest")       # align_corners means nothing here and torch refuses it


def yuv_444_to_420(yuv, mode: str = "avg_pool"):
    """[N,3,H,W], or three [N,1,H,W] planes -> (y, u, v) with u, v averaged over 2 x 2 blocks (mode "avg_pool", the only one)"""
    if mode not in DOWNSAMPLING:
        raise ValueError(f'Invalid downsampling mode "{mode}".')
    luma, u, v = yuv.split(1, dim=1) if isinstance(yuv, Tensor) else yuv
    return luma, _resample(u, mode), _resample(v, mode)


def yuv_420_to_444(yuv, mode: str = "bilinear", return_tuple: bool = False):
    """three planes [N,1,H,W], [N,1,H/2,W/2], [N,1,H/2,W/2] -> [N,3,H,W] (or the three full-size planes with return_tuple): chroma
    upsampled x2, "bilinear" (align_corners=False) or "nearest" """
    if len(yuv) != 3 or not all(isinstance(p, Tensor) for p in yuv):
        raise ValueError("Expected a tuple of 3 torch tensors")
    if mode not in UPSAMPLING:
        raise ValueError(f'Invalid upsampling mode "{mode}".')
    full = (yuv[0], _resample(yuv[1], mode), _resample(yuv[2], mode))
    return full if return_tuple else torch.cat(full, dim=1)


# ---- the fused pairs: HIP on device planes, the composition above on host planes
def yuv420_planes_to_rgb(yuv, bit_depth: int = 8, mode: str = "bilinear", clamp: bool = False) -> Tensor:
    """INTEGER 4:2:0 planes (y [N,1,H,W] or [N,H,W]; u, v half the size; uint8, or uint16 holding bit_depth bits) -> fp32 RGB
    [N,3,H,W] = ycbcr2rgb(yuv_420_to_444(planes / (2^bit_depth - 1), mode)).  Device planes: one stem_yuv420_to_rgb launch."""
    if len(yuv) != 3 or not all(isinstance(p, Tensor) for p in yuv):
        raise ValueError("Expected a tuple of 3 torch tensors")
    if mode not in UPSAMPLING:
        raise ValueError(f'Invalid upsampling mode "{mode}".')
    y, u, v = (c.squeeze(1) if c.dim() == 4 else c for c in yuv)
    if y.is_cuda:
        from . import functional
        return functional.yuv420_to_rgb(y, u, v, bit_depth=bit_depth, upsample=mode, clamp01=clamp)
    peak = float((1 << bit_depth) - 1)
    planes = tuple(torch.from_numpy(c.numpy().astype("float32")).unsqueeze(1) / peak for c in (y, u, v))     # uint16 has no .float()
    rgb = ycbcr2rgb(yuv_420_to_444(planes, mode=mode))
    return rgb.clamp_(0, 1) if clamp else rgb


def rgb_to_yuv420_planes(rgb: Tensor, bit_depth=None):
    """fp32 RGB [N,3,H,W] -> (y [N,H,W], u, v [N,H/2,W/2]) = yuv_444_to_420(rgb2ycbcr(rgb)); with bit_depth 8 | 10 quantised to
    uint8 | uint16 planes, rint(clamp(value, 0, 1) * (2^bit_depth - 1)).  Device tensors: one stem_rgb_to_yuv420 launch."""
    _image_channels(rgb)
    if rgb.dim() != 4:
        raise ValueError("Expected a 4D tensor with shape (Nx3xHxW) as input")
    if rgb.is_cuda:
        from . import functional
        return functional.rgb_to_yuv420(rgb.float(), bit_depth=bit_depth)
    y, u, v = (c.squeeze(1) for c in yuv_444_to_420(rgb2ycbcr(rgb)))
    if bit_depth is None:
        return y, u, v
    if bit_depth not in (8, 10):
        raise ValueError(f"bit_depth is 8 or 10, got {bit_depth!r}")
    peak, dt = float((1 << bit_depth) - 1), ("uint8" if bit_depth == 8 else "uint16")
    return tuple(torch.from_numpy(torch.round(c.double().clamp(0, 1) * peak).numpy().astype(dt)) for c in (y, u, v))


# ---- the callable forms: one class body, four bindings
class _Transform:
    """A transform function with its options fixed at construction.  Subclasses name the function, the options with their
    defaults (positional order = declaration order) and which options repr() shows."""
    function = None
    options: dict = {}
    shown: tuple = ()

    def __init__(self, *args, **kwargs):
        names = list(self.options)
        if len(args) > len(names) or set(kwargs) - set(names) or set(kwargs) & set(names[:len(args)]):
            raise TypeError(f"{type(self).__name__} takes the options {names}")
        given = {**dict(zip(names, args)), **kwargs}
        for name, default in self.options.items():
            setattr(self, name, type(default)(given.get(name, default)))

    def __call__(self, x):
        return type(self).function(x, **{name: getattr(self, name) for name in self.options})

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{name}={getattr(self, name)}' for name in self.shown)})"


class RGB2YCbCr(_Transform):
    """RGB tensor in [0,1], [3,H,W] or [N,3,H,W] -> YCbCr"""
    function = staticmethod(rgb2ycbcr)


class YCbCr2RGB(_Transform):
    """YCbCr tensor in [0,1], [3,H,W] or [N,3,H,W] -> RGB"""
    function = staticmethod(ycbcr2rgb)


class YUV444To420(_Transform):
    """[N,3,H,W] (or three [N,1,H,W] planes) -> (y [N,1,H,W], u, v [N,1,H/2,W/2]); mode: "avg_pool" """
    function = staticmethod(yuv_444_to_420)
    options = {"mode": "avg_pool"}


class YUV420To444(_Transform):
    """(y [N,1,H,W], u, v [N,1,H/2,W/2]) -> [N,3,H,W], or the three full-size planes with return_tuple; mode: "bilinear" | "nearest" """
    function = staticmethod(yuv_420_to_444)
    options = {"mode": "bilinear", "return_tuple": False}
    shown = ("return_tuple",)
