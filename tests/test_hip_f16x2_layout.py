"""The planes tensor and the packed weight images of the split-operand fp16 kernels, byte for byte, against a numpy restatement
of the layout that csrc/f16x3_layout.h states once (written here independently of it: scale exponent, the two fp16 planes of a
value, piece addresses, the XOR swizzle of a weight row, the phase order of a transposed face).  No tolerance anywhere: payload
bytes and words 0-1 of the scale record (slot count, 2^-e) are compared for equality.

Inputs are signed values m * 2^-20 * amax with integer m in [2^19, 2^20) and amax a power of two.  Then v * 2^e lies in
[2^14, 2^15) with 20 significant bits: the leading plane a0 = fp16(v 2^e) is a normal fp16 number, the residual v 2^e - a0 is a
multiple of 2^-5 below 2^3, i.e. exactly representable in fp32 and a normal fp16 number or zero -- no subnormal, no double
rounding, nothing on which a correct implementation and numpy could differ.  (Times a leaky-ReLU slope of 2^-2 the same holds
two binades lower.)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return functional


def exact_values(shape, seed, amax=1.0):
    rng = np.random.default_rng(seed)
    m = rng.integers(2 ** 19, 2 ** 20, size=shape).astype(np.float64)
    return (rng.choice([-1.0, 1.0], size=shape) * m * 2.0 ** -20 * amax).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def q_exp(bound):
    """e with bound * 2^e in [2^14, 2^15), from the exponent field of the fp32 bound"""
    b = int(np.float32(bound).view(np.uint32)) & 0x7FFFFFFF
    eb = (b >> 23) - 127
    if b == 0 or eb == 128:
        return 0
    return min(14 - max(eb, -126), 126)


def two_planes(v, e):
    xs = v.astype(np.float32) * np.float32(2.0 ** e)
    a0 = xs.astype(np.float16)
    return a0, (xs - a0.astype(np.float32)).astype(np.float16)


def planes_bytes(x_nhwc, e):
    """[pixel][C] fp32 -> payload: 16-byte piece p (8 channels) of slab sl (32 channels) of a pixel, plane pl, at
    pix * nslab * 128 + sl * 128 + pl * 64 + p * 16"""
    npix, Cc = x_nhwc.shape
    nslab = Cc // 32
    out = np.zeros(npix * nslab * 128 // 2, np.float16)
    pix, ch = np.arange(npix)[:, None], np.arange(Cc)[None, :]
    sl, p, c = ch // 32, (ch % 32) // 8, ch % 8
    for pl, a in enumerate(two_planes(x_nhwc, e)):
        out[(pix * nslab * 128 + sl * 128 + pl * 64 + p * 16 + c * 2) // 2] = a
    return out.view(np.uint8)


def image_bytes(wsel, rows, e):
    """wsel [N][C][T] (image rows, contraction channels, image taps) -> [N tile][chunk = slab * T + tap][plane][rows][64 B], piece
    p of row nl at nl * 64 + ((p ^ ((nl >> 2) & 3)) << 4); rows >= N are zero"""
    N, Cc, T = wsel.shape
    ntile, nslab = cdiv(N, rows), Cc // 32
    padded = np.zeros((ntile * rows, Cc, T), np.float32)
    padded[:N] = wsel
    out = np.zeros(ntile * nslab * T * 2 * rows * 64 // 2, np.float16)
    n, ch, tap = np.arange(ntile * rows)[:, None, None], np.arange(Cc)[None, :, None], np.arange(T)[None, None, :]
    nt, nl, sl, p, c = n // rows, n % rows, ch // 32, (ch % 32) // 8, ch % 8
    for pl, a in enumerate(two_planes(padded, e)):
        out[(((nt * nslab + sl) * T + tap) * 2 * rows * 64 + pl * rows * 64 + nl * 64 + ((p ^ ((nl >> 2) & 3)) << 4) + c * 2) // 2] = a
    return out.view(np.uint8)


def oriented(w, flip):
    """torch weight [K][C][R][S] -> [rows][contraction][tap]: as it stands, or (flip: the input gradient's operand) rows = C,
    contraction = K, taps mirrored"""
    K, Cc = w.shape[:2]
    w3 = w.reshape(K, Cc, -1)
    return w3.transpose(1, 0, 2)[:, :, ::-1] if flip else w3


def check_image(buf, expect, full_bytes, e, slots=64):
    got = buf.cpu().numpy()
    assert np.array_equal(got[:expect.size], expect), f"{int((got[:expect.size] != expect).sum())} payload bytes differ"
    rec = got[full_bytes:full_bytes + 8]
    assert int(rec[:4].view(np.int32)[0]) == slots and float(rec[4:].view(np.float32)[0]) == 2.0 ** -e


# ---- planes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_pitch", [False, True], ids=["dense", "view-of-96"])
@pytest.mark.parametrize("dact", [False, True], ids=["split", "split_dact"])
def test_planes_bytes(F, wide_pitch, dact):
    """70 pixels (more than one 64-pixel record slot) x 64 channels, from a dense tensor and from a 64-channel view of a
    96-channel buffer (pixel pitch > C); split_dact with z of mixed sign (zero counts as negative); merge(split(x)) == x."""
    B, Cc, H, W = 1, 64, 5, 14
    slope = 0.25
    x, z = exact_values((B, Cc, H, W), 1), exact_values((B, Cc, H, W), 2)
    z.reshape(-1)[::7] = 0.0
    xd = F.empty_nhwc(B, Cc, H, W, "cuda", ld=96 if wide_pitch else None)
    zd = F.empty_nhwc(B, Cc, H, W, "cuda", ld=96 if wide_pitch else None)
    xd.copy_(dev(x))
    zd.copy_(dev(z))
    assert F.nhwc_ld(xd) == (96 if wide_pitch else Cc)
    xp = F.F16Planes.split_dact(xd, zd, slope) if dact else F.F16Planes.split(xd)
    v = np.where(z > 0, x, x * np.float32(slope)) if dact else x
    e = q_exp(np.abs(x).max() * np.float32(max(1.0, abs(slope)) if dact else 1.0))
    npix = B * H * W
    expect = planes_bytes(v.transpose(0, 2, 3, 1).reshape(npix, Cc), e)
    # the record: one slot per workgroup of the maximum pass (2048 float4 each, at most one per 64-pixel x 128-channel tile)
    slots = min(max(cdiv(npix * (Cc // 4), 2048), 1), cdiv(npix, 64) * cdiv(Cc, 128), 1024)
    assert xp.q_offset == expect.size
    check_image(xp.data, expect, xp.q_offset, e, slots)
    merged = xp.merge().cpu().numpy()
    assert np.array_equal(merged.view(np.uint32), v.view(np.uint32))


# ---- weight images ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("N,Cc,R", [(40, 32, 3), (192, 64, 1)])
def test_wide_image_bytes(F, N, Cc, R, flip):
    """the 192-row image of conv_f16x3_kernel: one tile, all taps, rows >= N zero"""
    w = exact_values((Cc, N, R, R) if flip else (N, Cc, R, R), 3, 2.0 ** -3)
    e = q_exp(np.abs(w).max())
    expect = image_bytes(oriented(w, flip), 192, e)
    assert expect.size == (Cc // 32) * R * R * 2 * 192 * 64
    check_image(F.pack_weight_f16x2(dev(w), flip=flip), expect, expect.size, e)


@pytest.mark.parametrize("flip", [False, True])
def test_gen_image_bytes(F, flip):
    """the 128-row image: 130 rows = two N tiles, the second one two live rows"""
    N, Cc, R = 130, 64, 5
    w = exact_values((Cc, N, R, R) if flip else (N, Cc, R, R), 4, 2.0 ** -3)
    e = q_exp(np.abs(w).max())
    expect = image_bytes(oriented(w, flip), 128, e)
    assert expect.size == 2 * (Cc // 32) * R * R * 2 * 128 * 64
    check_image(F.pack_weight_f16x2_gen(dev(w), flip=flip), expect, expect.size, e)


def test_gen_image_masked_prefix(F):
    """taps = 12 of 25: the image holds the first 12 taps of every slab, its record stays behind the FULL image's size, the other
    taps of the source weight are zeroed in place and do not count for the scale"""
    N, Cc, R, taps = 8, 32, 5, 12
    w = exact_values((N, Cc, R, R), 5, 2.0 ** -3)
    w.reshape(N, Cc, -1)[0, 0, taps] = np.float32(0.25)      # the largest value sits in a masked tap
    wd = dev(w)
    buf = F.pack_weight_f16x2_gen(wd, taps=taps)
    live = w.reshape(N, Cc, -1)[:, :, :taps]
    e = q_exp(np.abs(live).max())
    check_image(buf, image_bytes(live, 128, e), (Cc // 32) * R * R * 2 * 128 * 64, e)
    after = wd.cpu().numpy().reshape(N, Cc, -1)
    assert np.array_equal(after[:, :, :taps], live) and not after[:, :, taps:].any()


def tconv_axis(R, pad, par):
    """taps r = par + pad (mod 2) of an R-tap axis: (count, largest r)"""
    rmin = (par + pad) & 1
    cnt = (R - 1 - rmin) // 2 + 1 if rmin < R else 0
    return cnt, rmin + 2 * (cnt - 1)


def test_multi_pack_phase_images(F):
    """flip = 2: the four sub-pixel phase images of a transposed face, phase 2 py + px behind phase 2 py + px - 1; phase (py, px)
    holds the taps r = py + pad, s = px + pad (mod 2) in descending r, then descending s (ascending offset on the coarse grid);
    the weight is read as w[c][n][r][s], taps not mirrored"""
    from spatiotemporalentropymodel_amd import _lib
    N, Cc, R = 64, 32, 3
    w = exact_values((Cc, N, R, R), 6, 2.0 ** -3)
    e = q_exp(np.abs(w).max())
    parts = []
    for ph in range(4):
        (cy, ry), (cx, rx) = tconv_axis(R, R // 2, ph >> 1), tconv_axis(R, R // 2, ph & 1)
        order = [(ry - 2 * jy) * R + (rx - 2 * jx) for jy in range(cy) for jx in range(cx)]
        parts.append(image_bytes(w.reshape(Cc, N, -1).transpose(1, 0, 2)[:, :, order], 128, e))
    expect = np.concatenate(parts)
    assert [p.size // (2 * 128 * 64) for p in parts] == [1, 2, 2, 4] and expect.size == R * R * 2 * 128 * 64
    wd = dev(w)
    out = torch.empty(F.f16x2_gen_weight_bytes(N, Cc, R, R), device="cuda", dtype=torch.uint8)
    F.pack_weights_f16x2_multi((_lib.F16PackDesc * 1)(_lib.F16PackDesc(wd.data_ptr(), out.data_ptr(), N, Cc, R, R, 2, 0)))
    check_image(out, expect, expect.size, e)
