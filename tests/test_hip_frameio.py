"""GPU, op level: the frame ingest / emit kernels (csrc/frameio.hip) against the two-pass compositions they replace,
    functional.yuv420_to_rgb_padded   ==  bitstream.pad(functional.yuv420_to_rgb(...), 64)
    functional.rgb_window_to_yuv420   ==  functional.rgb_to_yuv420(bitstream.crop(x, size).contiguous(), bit_depth)
bit for bit (torch.equal; the pad is +0.0 by its sign bit too).  The oracle is the existing code, never the new."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

#: h x w: one item, one row of items, W % 4 == 2, odd pad offsets (top = left = 1), no pad, top 31 / left 59, more than one workgroup
SIZES = [(2, 2), (2, 4), (6, 10), (62, 126), (64, 64), (66, 130), (120, 104)]
GUARD = 64                    # sentinel elements on either side of every output


def _planes(B, h, w, bits, seed):
    rng = np.random.default_rng(seed)
    dt, peak = (np.uint8, 255) if bits == 8 else (np.uint16, 1023)
    y, u, v = (rng.integers(0, peak + 1, size=s).astype(dt) for s in ((B, h, w), (B, h // 2, w // 2), (B, h // 2, w // 2)))
    y[0, 0, 0], y[0, -1, -1] = 0, peak                          # the extremes, so that clamp01 has something to clamp
    u[0, 0, 0], v[0, 0, 0], u[0, -1, -1], v[0, -1, -1] = 0, peak, peak, 0
    return tuple(torch.from_numpy(a).cuda() for a in (y, u, v))


def _same_ints(a, b):
    """torch.equal of two integer planes of one type (compared as int32: every torch build compares those)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.to(torch.int32), b.to(torch.int32))


def _ingest_into_guarded(y, u, v, bits, upsample, clamp01, frame):
    """the kernel writing into the middle of a NaN-poisoned buffer with sentinels on both sides -> (frame tensor, the guards)"""
    from spatiotemporalentropymodel_amd import _lib
    from spatiotemporalentropymodel_amd import functional as F
    B, h, w = y.shape
    Hp, Wp, top, left = frame
    n = B * 3 * Hp * Wp
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    out = buf[GUARD:GUARD + n].view(B, 3, Hp, Wp)
    _lib.check_frameio(_lib.frameio().stem_yuv420_to_rgb_padded(y.data_ptr(), u.data_ptr(), v.data_ptr(), B, h, w, y.element_size(), bits,
                                                               F.YUV_UPSAMPLE[upsample], int(clamp01), out.data_ptr(), Hp, Wp, top, left,
                                                               F._stream()))
    return out, torch.cat([buf[:GUARD], buf[GUARD + n:]])


def _assert_same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), what
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: equal values, other bits (a -0.0 in the pad?)"


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ingest_equals_convert_then_pad(hw, B, bits):
    from spatiotemporalentropymodel_amd import bitstream
    from spatiotemporalentropymodel_amd import functional as F
    h, w = hw
    y, u, v = _planes(B, h, w, bits, seed=h * 1000 + w + bits)
    for upsample in ("bilinear", "nearest"):
        for clamp01 in (True, False):
            want = bitstream.pad(F.yuv420_to_rgb(y, u, v, bits, upsample, clamp01), 64)
            got = F.yuv420_to_rgb_padded(y, u, v, bits, upsample, clamp01, multiple=64)
            _assert_same_bits(got, want, (hw, B, bits, upsample, clamp01))
            frame = F.pad_geometry(h, w, 64)
            out, guards = _ingest_into_guarded(y, u, v, bits, upsample, clamp01, frame)
            _assert_same_bits(out, want, ("poisoned", hw, B, bits, upsample, clamp01))
            assert torch.isnan(guards).all(), "the kernel wrote outside its frame"
            again, _ = _ingest_into_guarded(y, u, v, bits, upsample, clamp01, frame)
            _assert_same_bits(again, out, "relaunch")


@pytest.mark.parametrize("frame", [(10, 14, 0, 0), (10, 14, 4, 4), (9, 13, 3, 0), (7, 11, 0, 1), (6, 10, 0, 0), (70, 75, 63, 1)],
                         ids=lambda f: "Hp%d_Wp%d_top%d_left%d" % f)
@pytest.mark.parametrize("bits", [8, 10])
def test_ingest_explicit_frame_with_the_image_in_a_corner(frame, bits):
    """frames whose sides are no multiples of anything, the image flush with each corner, odd Wp (no vector access is legal)"""
    from spatiotemporalentropymodel_amd import functional as F
    Hp, Wp, top, left = frame
    h, w = 6, 10
    y, u, v = _planes(2, h, w, bits, seed=7 + Hp)
    for upsample in ("bilinear", "nearest"):
        want = torch.zeros((2, 3, Hp, Wp), device="cuda")
        want[:, :, top:top + h, left:left + w] = F.yuv420_to_rgb(y, u, v, bits, upsample, True)
        out, guards = _ingest_into_guarded(y, u, v, bits, upsample, True, frame)
        _assert_same_bits(out, want, (frame, bits, upsample))
        assert torch.isnan(guards).all()
        _assert_same_bits(F.yuv420_to_rgb_padded(y, u, v, bits, upsample, True, frame=frame), want, "wrapper")


def _rgb_frame(B, Hp, Wp, seed, peak):
    """values inside and outside [0, 1], and values whose luma / chroma land exactly on rounding ties: grey pixels k + 0.5 steps"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.25, 1.25, size=(B, 3, Hp, Wp)).astype(np.float32)
    ties = ((np.arange(Wp) % 64) + 0.5) / peak                                       # r = g = b -> y = that value up to fp64 rounding
    x[:, :, 0::3, :] = ties.astype(np.float32)[None, None, None, :]
    x[:, :, 1::7, :] = np.float32(0.5)                                               # chroma exactly 0.5: peak / 2 is a tie for odd peaks
    return torch.from_numpy(x).cuda()


def _emit_into_guarded(x, size, origin, bits):
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
    _lib.check_frameio(_lib.frameio().stem_rgb_window_to_yuv420(x.data_ptr(), B, Hp, Wp, x.stride(2), x.stride(1), origin[0], origin[1], h, w,
                                                               yo.data_ptr(), uo.data_ptr(), vo.data_ptr(), yo.element_size(), bits, F._stream()))
    keep = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    for a, n in ((GUARD, ny), (2 * GUARD + ny, nc), (3 * GUARD + ny + nc, nc)):
        keep[a:a + n] = False
    guards = buf.to(torch.int32)[keep]
    return (yo.view(B, h, w), uo.view(B, h // 2, w // 2), vo.view(B, h // 2, w // 2)), bool((guards == sentinel).all())


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_emit_equals_crop_then_convert(hw, B, bits):
    from spatiotemporalentropymodel_amd import bitstream
    from spatiotemporalentropymodel_amd import functional as F
    h, w = hw
    Hp, Wp, top, left = F.pad_geometry(h, w, 64)
    x = _rgb_frame(B, Hp, Wp, seed=h * 100 + w, peak=(1 << bits) - 1)
    want = F.rgb_to_yuv420(bitstream.crop(x, (h, w)).contiguous(), bits)
    got = F.rgb_window_to_yuv420(x, (h, w), bits)
    for a, b, name in zip(got, want, "yuv"):
        assert _same_ints(a, b), (name, hw, B, bits)
    planes, clean = _emit_into_guarded(x, (h, w), (top, left), bits)
    assert clean, "the kernel wrote outside its planes"
    again, _ = _emit_into_guarded(x, (h, w), (top, left), bits)
    for a, b, c in zip(planes, want, again):
        assert _same_ints(a, b) and _same_ints(a, c)


@pytest.mark.parametrize("origin", [(0, 0), (1, 0), (0, 1), (3, 5), (4, 8), (10, 22)], ids=lambda o: "top%d_left%d" % o)
@pytest.mark.parametrize("bits", [8, 10])
def test_emit_windows_views_and_whole_frames(origin, bits):
    """odd and even offsets (the 2 x 2 blocks follow the window), h = 2, the window that is the whole frame, and the frame as a view of
    a wider and taller tensor (row pitch > Wp, plane pitch > Hp * Wp)"""
    from spatiotemporalentropymodel_amd import functional as F
    top, left = origin
    Hp, Wp = 20, 40
    big = _rgb_frame(2, Hp + 3, Wp + 12, seed=11 + top, peak=(1 << bits) - 1)
    view = big[:, :, 2:2 + Hp, 4:4 + Wp]                                              # row pitch Wp + 12, first element 16-byte aligned or not
    assert not view.is_contiguous()
    for x in (view.contiguous(), view):
        for h, w in ((2, 18), (10, 18), (10, 16)):
            want = F.rgb_to_yuv420(x[:, :, top:top + h, left:left + w].contiguous(), bits)
            planes, clean = _emit_into_guarded(x, (h, w), origin, bits)
            assert clean
            for a, b in zip(planes, want):
                assert _same_ints(a, b), (origin, bits, h, w, x.is_contiguous())
            for a, b in zip(F.rgb_window_to_yuv420(x, (h, w), bits, origin=origin), want):
                assert _same_ints(a, b)
    whole = view.contiguous()
    for a, b in zip(F.rgb_window_to_yuv420(whole, (Hp, Wp), bits), F.rgb_to_yuv420(whole, bits)):
        assert _same_ints(a, b)


def test_refusals_come_before_any_launch():
    """wrong geometry through the wrappers: ValueError / RuntimeError with the outputs untouched (nothing was launched)"""
    from spatiotemporalentropymodel_amd import _lib
    from spatiotemporalentropymodel_amd import functional as F
    y, u, v = _planes(1, 6, 10, 8, seed=3)
    with pytest.raises(ValueError, match="does not fit"):
        F.yuv420_to_rgb_padded(y, u, v, 8, frame=(6, 10, 1, 0))
    with pytest.raises(ValueError, match="even sides"):
        F.yuv420_to_rgb_padded(y[:, :5], u, v, 8)
    x = torch.zeros((1, 3, 64, 64), device="cuda")
    with pytest.raises(ValueError, match="does not fit"):
        F.rgb_window_to_yuv420(x, (6, 10), 8, origin=(60, 0))
    with pytest.raises(ValueError, match="even sides"):
        F.rgb_window_to_yuv420(x, (5, 10), 8)
    with pytest.raises(ValueError, match="bit_depth"):
        F.rgb_window_to_yuv420(x, (6, 10), 9)
    out = torch.full((3 * 64 * 64,), float("nan"), device="cuda")
    f = _lib.frameio()
    rc = f.stem_yuv420_to_rgb_padded(y.data_ptr(), u.data_ptr(), v.data_ptr(), 1, 6, 10, 1, 8, 0, 1, out.data_ptr(), 64, 64, 59, 0, F._stream())
    assert rc == -1 and b"does not fit" in f.stem_frameio_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
