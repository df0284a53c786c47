"""GPU, op level: the per-frame passes of the pixel-domain sequence codec (csrc/roiio.hip) bit for bit against what they replace --
rgb_window_recondition against bitstream.pad(bitstream.crop(.)) and the emit kernel's planes, roi_map_padded against the numpy float32
statement in tests/roi_map_ref.py.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import roi_map_ref

pytestmark = pytest.mark.gpu
GUARD = 64


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_ints(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.to(torch.int32), b.to(torch.int32))


def _rgb_frame(B, Hp, Wp, seed, peak):
    """values inside and outside [0, 1], rounding ties of luma and chroma, and negative zeros and NaN-free noise in what becomes border"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.25, 1.25, size=(B, 3, Hp, Wp)).astype(np.float32)
    ties = ((np.arange(Wp) % 64) + 0.5) / peak
    x[:, :, 0::3, :] = ties.astype(np.float32)[None, None, None, :]
    x[:, :, 1::7, :] = np.float32(0.5)
    x[:, :, :, 0::5] *= np.float32(-1.0)
    return torch.from_numpy(x).cuda()


def _recondition_guarded(x, size, origin, bits):
    """the entry point itself with the planes inside one buffer of sentinels -> (planes, the sentinels survived)"""
    from spatiotemporalentropymodel_amd import _lib
    from spatiotemporalentropymodel_amd import functional as F
    B, _, Hp, Wp = x.shape
    h, w = size
    dt = torch.uint8 if bits == 8 else torch.uint16
    sentinel = 0xA5 if bits == 8 else 0xA5A5
    ny, nc = B * h * w, B * (h // 2) * (w // 2)
    buf = torch.full((ny + 2 * nc + 4 * GUARD,), sentinel, dtype=torch.int32, device="cuda").to(dt)
    yo = buf[GUARD:GUARD + ny]
    uo = buf[2 * GUARD + ny:2 * GUARD + ny + nc]
    vo = buf[3 * GUARD + ny + nc:3 * GUARD + ny + 2 * nc]
    _lib.check_roiio(_lib.roiio().stem_rgb_window_recondition(x.data_ptr(), B, Hp, Wp, x.stride(2), x.stride(1), origin[0], origin[1], h, w,
                                                             yo.data_ptr(), uo.data_ptr(), vo.data_ptr(), yo.element_size(), bits, F._stream()))
    keep = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    for a, n in ((GUARD, ny), (2 * GUARD + ny, nc), (3 * GUARD + ny + nc, nc)):
        keep[a:a + n] = False
    guards = buf.to(torch.int32)[keep]
    return (yo.view(B, h, w), uo.view(B, h // 2, w // 2), vo.view(B, h // 2, w // 2)), bool((guards == sentinel).all())


# (h, w), (Hp, Wp), B: the centred geometry of bitstream.pad; 6 x 10 sits at (29, 27), 122 x 126 at the odd offsets (3, 1), 64 x 64 has no
# border, 100 x 252 in 128 x 256 has top 14, left 2 (a multiple of four wide, not four aligned) and more than one workgroup of each kind
CASES = [((6, 10), (64, 64), 1), ((122, 126), (128, 128), 1), ((64, 64), (64, 64), 1), ((6, 10), (64, 64), 2), ((122, 126), (128, 128), 2),
         ((100, 252), (128, 256), 1), ((60, 64), (64, 64), 2)]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("hw,frame,B", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"B{v}")
def test_recondition_is_crop_pad_and_the_emit_kernels_planes(hw, frame, B, bits):
    from spatiotemporalentropymodel_amd import bitstream
    from spatiotemporalentropymodel_amd import functional as F
    h, w = hw
    Hp, Wp = frame
    assert F.pad_geometry(h, w, 64)[:2] == (Hp, Wp)
    before = _rgb_frame(B, Hp, Wp, seed=h * 100 + w + B, peak=(1 << bits) - 1)
    want_frame = _bits(bitstream.pad(bitstream.crop(before, (h, w)), 64))
    want_planes = F.rgb_window_to_yuv420(before, (h, w), bits)
    # with planes
    x = before.clone()
    got = F.rgb_window_recondition(x, (h, w), bits)
    assert torch.equal(_bits(x), want_frame)
    for a, b, name in zip(got, want_planes, "yuv"):
        assert torch.equal(a, b), (name, hw, B, bits)
    # a second launch changes nothing, in the frame or in the planes
    again = F.rgb_window_recondition(x, (h, w), bits)
    assert torch.equal(_bits(x), want_frame)
    for a, b in zip(again, want_planes):
        assert torch.equal(a, b)
    # planes NULL: the frame alone
    x = before.clone()
    assert F.rgb_window_recondition(x, (h, w)) is None
    assert torch.equal(_bits(x), want_frame)
    assert F.rgb_window_recondition(x, (h, w)) is None and torch.equal(_bits(x), want_frame)
    # the entry point, planes between sentinels
    x = before.clone()
    planes, clean = _recondition_guarded(x, (h, w), F.pad_geometry(h, w, 64)[2:], bits)
    assert clean, "the kernel wrote outside its planes"
    assert torch.equal(_bits(x), want_frame)
    for a, b in zip(planes, want_planes):
        assert _same_ints(a, b)


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("origin", [(0, 0), (1, 0), (3, 5), (4, 8), (10, 22)], ids=lambda o: "top%d_left%d" % o)
def test_recondition_of_a_pitched_view_leaves_the_gap_alone(origin, bits):
    """the frame as a view of a wider and taller tensor (row pitch > Wp, plane pitch > Hp * Wp): everything of the larger tensor outside
    the view is a sentinel before and after; windows at odd and even offsets, h = 2, and the window that is the whole frame"""
    from spatiotemporalentropymodel_amd import functional as F
    top, left = origin
    Hp, Wp = 20, 40
    inner = _rgb_frame(2, Hp, Wp, seed=11 + top, peak=(1 << bits) - 1)
    for h, w in ((2, 18), (10, 18), (10, 16), (Hp, Wp)):
        if (h, w) == (Hp, Wp):
            top, left = 0, 0
        big = torch.full((2, 3, Hp + 3, Wp + 12), 7.5, device="cuda")
        view = big[:, :, 2:2 + Hp, 4:4 + Wp]
        view.copy_(inner)
        assert not view.is_contiguous()
        want_planes = F.rgb_window_to_yuv420(inner, (h, w), bits, origin=(top, left))
        want = torch.zeros_like(inner)
        want[:, :, top:top + h, left:left + w] = inner[:, :, top:top + h, left:left + w]
        for with_planes in (True, False):
            view.copy_(inner)
            got = F.rgb_window_recondition(view, (h, w), bits if with_planes else None, origin=(top, left))
            assert torch.equal(_bits(view), _bits(want)), (origin, h, w, with_planes)
            outside = torch.ones_like(big, dtype=torch.bool)
            outside[:, :, 2:2 + Hp, 4:4 + Wp] = False
            assert bool((big[outside] == 7.5).all()), "the kernel wrote into the pitch gap"
            if with_planes:
                for a, b in zip(got, want_planes):
                    assert torch.equal(a, b), (origin, h, w)
            else:
                assert got is None


def test_recondition_refusals_come_before_any_launch():
    from spatiotemporalentropymodel_amd import _lib
    from spatiotemporalentropymodel_amd import functional as F
    x = torch.full((1, 3, 64, 64), float("nan"), device="cuda")
    with pytest.raises(ValueError, match="does not fit"):
        F.rgb_window_recondition(x, (6, 10), 8, origin=(60, 0))
    with pytest.raises(ValueError, match="even sides"):
        F.rgb_window_recondition(x, (5, 10), 8)
    with pytest.raises(ValueError, match="bit_depth"):
        F.rgb_window_recondition(x, (6, 10), 9)
    with pytest.raises(ValueError, match="in place"):
        F.rgb_window_recondition(x.permute(0, 1, 3, 2), (6, 10))
    with pytest.raises(TypeError):
        F.rgb_window_recondition(x.double(), (6, 10))
    r = _lib.roiio()
    y = torch.zeros(64, dtype=torch.uint8, device="cuda")
    rc = r.stem_rgb_window_recondition(x.data_ptr(), 1, 64, 64, 64, 64 * 64, 59, 0, 6, 10, y.data_ptr(), y.data_ptr(), y.data_ptr(), 1, 8, F._stream())
    assert rc == -1 and b"does not fit" in r.stem_roiio_last_error()
    rc = r.stem_rgb_window_recondition(x.data_ptr(), 1, 64, 64, 64, 64 * 64, 29, 27, 6, 10, y.data_ptr(), None, y.data_ptr(), 1, 8, F._stream())
    assert rc == -1 and b"all given or all NULL" in r.stem_roiio_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(x).all()


# ---- the rasteriser ----------------------------------------------------------------------------------------------------------------
def _rng_boxes(n, h, w, seed):
    """n boxes with arbitrary (non-dyadic) values and feathers, some reaching outside the window"""
    rng = np.random.default_rng(seed)
    boxes = []
    for _ in range(n):
        x0, y0 = int(rng.integers(-w // 4, w)), int(rng.integers(-h // 4, h))
        x1, y1 = x0 + int(rng.integers(1, w // 2 + 2)), y0 + int(rng.integers(1, h // 2 + 2))
        boxes.append((x0, y0, x1, y1, float(np.float32(rng.uniform(0, 1))), int(rng.integers(0, 12))))
    return boxes


def _check_map(boxes, size, background, **kw):
    from spatiotemporalentropymodel_amd import functional as F
    got = F.roi_map_padded(boxes, size, background, device="cuda:0", **kw)
    want = roi_map_ref.roi_map_padded(boxes, size, background, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (size, kw)
    return got


@pytest.mark.parametrize("name", list(roi_map_ref.EXACT_CASES))
def test_roi_map_on_the_cpu_tests_cases(name):
    boxes, size, background = roi_map_ref.EXACT_CASES[name]
    _check_map(boxes, size, background)
    _check_map(boxes, size, background, frame=(size[0] + 5, size[1] + 3, 2, 1))


@pytest.mark.parametrize("hw,n", [((6, 10), 5), ((64, 64), 64), ((122, 126), 64), ((128, 128), 17), ((100, 200), 1)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"n{v}")
def test_roi_map_with_arbitrary_values(hw, n):
    """values, backgrounds and feathers whose blends round: the kernel's three roundings and its division are numpy's"""
    boxes = _rng_boxes(n, *hw, seed=hw[0] * 7 + n)
    _check_map(boxes, hw, float(np.float32(0.3)))
    if hw == (6, 10):
        for frame in ((9, 13, 2, 1), (7, 11, 0, 1), (6, 10, 0, 0), (64, 70, 29, 30)):   # Wp no multiple of four: element-wise stores
            _check_map(boxes, hw, float(np.float32(0.7)), frame=frame)


def test_roi_map_of_a_1080p_frame_is_one_launch_and_overwrites_everything():
    from spatiotemporalentropymodel_amd import functional as F
    boxes = [(200, 100, 900, 700, 0.9, 32), (600, 400, 1900, 1079, 0.65, 15), (-50, -50, 120, 90, 1.0, 7), (1000, 500, 1100, 600, 0.1)] + \
        _rng_boxes(60, 1080, 1920, seed=5)
    got = _check_map(boxes, (1080, 1920), float(np.float32(0.45)))
    assert tuple(got.shape) == (1, 1, 1088, 1920)
    # a NaN-prefilled output through the entry point comes back clean: every element is written
    from spatiotemporalentropymodel_amd import _lib
    geo, values, background = F.roi_boxes_check(boxes[:9], 0.45)
    for (h, w), (Hp, Wp, top, left) in (((1080, 1920), (1088, 1920, 4, 0)), ((6, 10), (64, 64, 29, 27)), ((6, 10), (9, 13, 2, 1))):
        out = torch.full((1, 1, Hp, Wp), float("nan"), device="cuda")
        b = torch.tensor(geo, dtype=torch.int32, device="cuda")
        v = torch.tensor(values, dtype=torch.float32, device="cuda")
        _lib.check_roiio(_lib.roiio().stem_roi_map_padded(b.data_ptr(), v.data_ptr(), len(geo), background, out.data_ptr(), Hp, Wp, top, left, h, w,
                                                         F._stream()))
        want = roi_map_ref.roi_map_padded(boxes[:9], (h, w), np.float32(0.45), frame=(Hp, Wp, top, left))
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    empty = torch.full((1, 1, 64, 64), float("nan"), device="cuda")
    _lib.check_roiio(_lib.roiio().stem_roi_map_padded(None, None, 0, 0.25, empty.data_ptr(), 64, 64, 29, 27, 6, 10, F._stream()))
    assert np.array_equal(empty.cpu().numpy(), roi_map_ref.roi_map_padded([], (6, 10), 0.25))
