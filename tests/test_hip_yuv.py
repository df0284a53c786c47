"""GPU: the YUV 4:2:0 kernels (csrc/yuv.hip) against the reference's float64 results (tests/golden/yuv_transforms*.npz, written by
tests/golden/make_golden_yuv.py from compressai/transforms/functional.py), the sequence reader / writer on top of them and
evaluation.eval_gop(yuv=True).

The float gate is absolute and derived, not tuned: the reference's chain is at most ten fp32 roundings of 2^-24 on magnitudes <= 2
(full-range random chroma drives r, g, b to about +-2), and the division by K_g = 0.7152 amplifies what reaches g by 1.4:
10 * 2 * 2^-24 * 1.4 = 1.7e-6 -> 2e-6.  The reference's own float32 arrays are asserted to lie within it."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GATE = 2e-6
HALF = 1e-4                    # a quantised sample may differ from rint(float64) only this close to a half-integer ...
EXCUSED_SHARE = 1e-3           # ... by one step, and on at most 0.1 % of a case's samples


import yuv_fixture as MOD  # noqa: E402

G = MOD.load()
CASES = [c for c, _ in MOD.cases(G)]


@pytest.fixture(scope="module")
def g():
    return G


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _bits(case):
    return int(case.split("_")[1])


def _planes(g, case, dev):
    return tuple(torch.from_numpy(g[f"{case}/{n}"]).to(dev) for n in "yuv")


def _border(a):
    """first and last rows and columns of [..., H, W] (where the interpolation taps clamp), as one vector"""
    return np.concatenate([a[..., 0, :].ravel(), a[..., -1, :].ravel(), a[..., :, 0].ravel(), a[..., :, -1].ravel()])


def _assert_integer_planes(got, exact, ref32, peak, what):
    """got: the kernel's integer plane; exact: the float64 plane in [0,1] units; ref32: the reference's float32 plane"""
    scaled = np.clip(exact, 0.0, 1.0) * peak
    want = np.rint(scaled)
    diff = got.astype(np.float64) - want
    bad = diff != 0
    dist = np.abs(scaled - np.floor(scaled) - 0.5)
    print(f"[yuv] {what}: {int(bad.sum())}/{bad.size} samples differ from rint(float64)")
    assert (np.abs(diff[bad]) == 1).all() and (dist[bad] <= HALF).all(), f"{what}: a sample differs away from a half-integer"
    assert bad.mean() <= EXCUSED_SHARE, what
    if ref32 is not None:                                  # the inputs are well chosen: the reference's float32 run stays within the share
        assert (MOD.quantise(ref32, peak) != want).mean() <= EXCUSED_SHARE, f"{what}: the inputs are badly chosen"


def _float_gate(got, exact, ref32, what):
    """every element and, separately, the edge rows / columns within GATE of float64; so is the reference's float32 run, where kept"""
    assert got.shape == exact.shape and got.dtype == np.float32, what
    err = np.abs(got - exact)
    ref_err = None if ref32 is None else np.abs(ref32.astype(np.float64) - exact).max()
    print(f"[yuv] {what}: HIP vs float64 {err.max():.2e} (border {_border(err).max():.2e})   reference-fp32 vs float64 "
          f"{'not kept' if ref_err is None else format(ref_err, '.2e')}   gate {GATE:.0e}")
    assert ref_err is None or ref_err <= GATE, "the gate is not reachable by the reference's own float32 run"
    assert _border(err).max() <= GATE, f"{what}: edge rows / columns (clamped taps)"
    assert err.max() <= GATE, what


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("case", CASES)
def test_yuv420_to_rgb_matches_float64(g, dev, case, mode):
    from spatiotemporalentropymodel_amd import functional as F
    ref = g[f"{case}/ref_images"]
    full = F.yuv420_to_rgb(*_planes(g, case, dev), bit_depth=_bits(case), upsample=mode, clamp01=False).cpu().numpy()
    _float_gate(full[ref], g[f"{case}/rgb64_{mode}"], g.get(f"{case}/rgb32_{mode}"), f"{case} {mode}")
    clamped = F.yuv420_to_rgb(*_planes(g, case, dev), bit_depth=_bits(case), upsample=mode, clamp01=True).cpu().numpy()
    assert np.array_equal(clamped, np.clip(full, 0.0, 1.0))


@pytest.mark.parametrize("case", CASES)
def test_rgb_to_yuv420_matches_float64(g, dev, case):
    from spatiotemporalentropymodel_amd import functional as F
    bits, ref = _bits(case), g[f"{case}/ref_images"]
    peak = float((1 << bits) - 1)
    src = torch.from_numpy(g[f"{case}/src"]).to(dev)
    flt = [p.cpu().numpy() for p in F.rgb_to_yuv420(src)]
    itg = [p.cpu().numpy() for p in F.rgb_to_yuv420(src, bit_depth=bits)]
    for n, a, q in zip("yuv", flt, itg):
        exact, ref32 = g[f"{case}/{n}64"], g.get(f"{case}/{n}32")
        assert q.shape == a.shape and q.dtype == (np.uint8 if bits == 8 else np.uint16)
        _float_gate(a[ref], exact, ref32, f"{case} {n}")
        _assert_integer_planes(q[ref], exact, ref32, peak, f"{case} {n}")


@pytest.mark.parametrize("case", CASES)
def test_transforms_single_steps_on_device_tensors(g, dev, case):
    """transforms.rgb2ycbcr / ycbcr2rgb / yuv_444_to_420 / yuv_420_to_444 and the class forms on fp32 DEVICE tensors (stem_ycbcr_convert,
    stem_plane_resample2: fp32, the reference's order of operations) against the same float64 arrays and the same gate; the
    nearest class form against the NEAREST arrays (the constructor's mode is the mode used)."""
    from spatiotemporalentropymodel_amd import transforms as T
    bits, ref = _bits(case), g[f"{case}/ref_images"]
    peak = float((1 << bits) - 1)
    planes = tuple((torch.from_numpy(g[f"{case}/{n}"].astype(np.float32)) / peak).unsqueeze(1).to(dev) for n in "yuv")
    for mode in ("bilinear", "nearest"):
        got = T.ycbcr2rgb(T.yuv_420_to_444(planes, mode=mode))
        assert got.is_cuda
        _float_gate(got.cpu().numpy()[ref], g[f"{case}/rgb64_{mode}"], g.get(f"{case}/rgb32_{mode}"), f"{case} transforms {mode}")
        again = T.YCbCr2RGB()(T.YUV420To444(mode=mode)(planes))
        assert torch.equal(again, got)
        y, u, v = T.yuv_420_to_444(planes, mode=mode, return_tuple=True)
        assert y is planes[0] and u.shape == y.shape == v.shape
    src = torch.from_numpy(g[f"{case}/src"]).to(dev)
    got = T.yuv_444_to_420(T.rgb2ycbcr(src))
    for n, p, q in zip("yuv", got, T.YUV444To420()(T.RGB2YCbCr()(src))):
        assert p.is_cuda and torch.equal(p, q)
        _float_gate(p.squeeze(1).cpu().numpy()[ref], g[f"{case}/{n}64"], g.get(f"{case}/{n}32"), f"{case} transforms {n}")
    one = T.rgb2ycbcr(src[0])                                          # 3-D input
    assert one.shape == src[0].shape and torch.equal(one, T.rgb2ycbcr(src)[0])
    for a, b in zip(T.yuv_444_to_420(tuple(T.rgb2ycbcr(src).split(1, 1))), got):     # the tuple form
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", [c for c in CASES if c.split("_")[0] in ("34x70", "66x258", "4x1028", "2x2")])
def test_squared_error_sums_are_exact_per_image_and_plane(g, dev, case):
    """sse[b][plane] against numpy's int64 sum over the kernel's own integer planes and the source planes; the B images carry errors
    of different sizes (image b's source is the quantised frame shifted by b + 1 steps on Y, 2b + 3 on U, 5 on V where it fits)"""
    from spatiotemporalentropymodel_amd import functional as F
    bits = _bits(case)
    peak = (1 << bits) - 1
    src = torch.from_numpy(g[f"{case}/src"]).to(dev)
    own = [p.cpu().numpy().astype(np.int64) for p in F.rgb_to_yuv420(src, bit_depth=bits)]
    B = own[0].shape[0]
    rng = np.random.default_rng(7)
    source = []
    for k, p in enumerate(own):
        step = np.array([(b + 1, 2 * b + 3, 5)[k] for b in range(B)]).reshape(B, 1, 1)
        s = np.clip(p + step * rng.integers(-1, 2, size=p.shape), 0, peak)
        source.append(s)
    dt = np.uint8 if bits == 8 else np.uint16
    y, u, v, sse = F.rgb_to_yuv420(src, bit_depth=bits, source=tuple(torch.from_numpy(s.astype(dt)).to(dev) for s in source))
    assert sse.dtype == torch.int64 and tuple(sse.shape) == (B, 3)
    for p, q in zip((y, u, v), own):
        assert np.array_equal(p.cpu().numpy(), q)                       # the planes do not depend on whether sums are taken
    want = np.stack([((p - s) ** 2).reshape(B, -1).sum(1) for p, s in zip(own, source)], axis=1)
    assert np.array_equal(sse.cpu().numpy(), want), (sse.cpu().numpy(), want)
    assert B == 1 or len({int(x) for x in want[:, 0]}) == B            # the images really differ
    # the frame against its own planes: exactly zero
    _, _, _, zero = F.rgb_to_yuv420(src, bit_depth=bits, source=(y, u, v))
    assert not zero.any()


@pytest.mark.parametrize("case", CASES)
def test_luma_round_trips_bit_for_bit(g, dev, case):
    """planes -> RGB (unclamped) -> planes gives back Y exactly (the conversion is exact to ~1e-7 of a step count of at most 1023);
    chroma went through a 2x upsampling and a 2x2 average and is not expected to"""
    from spatiotemporalentropymodel_amd import functional as F
    bits = _bits(case)
    planes = _planes(g, case, dev)
    for mode in ("bilinear", "nearest"):
        rgb = F.yuv420_to_rgb(*planes, bit_depth=bits, upsample=mode, clamp01=False)
        y, u, v = F.rgb_to_yuv420(rgb, bit_depth=bits)
        assert torch.equal(y, planes[0]), (case, mode)
        if mode == "nearest":                                           # the average of four copies: chroma round-trips too
            assert torch.equal(u, planes[1]) and torch.equal(v, planes[2])


def test_functional_checks_shapes_and_types(dev):
    from spatiotemporalentropymodel_amd import functional as F
    y, u = torch.zeros(1, 4, 6, dtype=torch.uint8, device=dev), torch.zeros(1, 2, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        F.yuv420_to_rgb(y[:, :3], u, u)                                 # odd height
    with pytest.raises(ValueError):
        F.yuv420_to_rgb(y, u[:, :1], u)
    with pytest.raises(ValueError):
        F.yuv420_to_rgb(y, u, u, bit_depth=10)                          # 10 bits do not fit uint8
    with pytest.raises(ValueError):
        F.yuv420_to_rgb(y, u, u, upsample="bicubic")
    with pytest.raises(TypeError):
        F.yuv420_to_rgb(y.float(), u, u)
    with pytest.raises(ValueError):
        F.rgb_to_yuv420(torch.zeros(1, 3, 5, 6, device=dev))
    with pytest.raises(ValueError):
        F.rgb_to_yuv420(torch.zeros(1, 3, 4, 6, device=dev), bit_depth=12)
    with pytest.raises(ValueError):
        F.rgb_to_yuv420(torch.zeros(1, 3, 4, 6, device=dev), source=(y, u, u))


@pytest.mark.parametrize("bits", [8, 10])
def test_written_file_reads_back_as_the_kernels_planes(tmp_path, dev, bits):
    from spatiotemporalentropymodel_amd import data, functional as F
    h, w = 34, 70
    x = torch.rand(3, 3, h, w, device=dev)
    want = F.rgb_to_yuv420(x, bit_depth=bits)
    path = tmp_path / "dec.yuv"
    data.write_yuv420(path, x[:2], bit_depth=bits, append=False)
    data.write_yuv420(path, x[2], bit_depth=bits)
    seq = data.YUVSequence(path, w, h, bit_depth=bits, device=dev, clamp=False)
    frames = list(seq)
    assert len(frames) == 3
    for b, f in enumerate(frames):
        assert f.shape == (3, h, w) and f.is_cuda and f.bit_depth == bits
        for p, q in zip(f.yuv_planes, want):
            assert torch.equal(p[0], q[b])
        assert torch.equal(f, F.yuv420_to_rgb(*f.yuv_planes, bit_depth=bits, clamp01=False)[0])


def test_eval_gop_yuv_psnr(golden, dev, tmp_path):
    """eval_gop(yuv=True, write_to=...) on the models and frames of tests/test_hip_codec.py::test_eval_gop_chain_matches_reference: the
    codec's results are those of a yuv=False run, and the four new numbers are what numpy computes from the written file and the
    source planes (plain RGB frames: the source is the frame quantised at 8 bits)."""
    from test_hip_codec import _eval_gop_models
    from spatiotemporalentropymodel_amd import data, evaluation, functional as F
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    gg = golden("eval_gop.npz")
    imodel, stem = _eval_gop_models(gg, dev)
    h, w = (int(v) for v in gg["size"])
    n = int(gg["nframes"][0])
    frames = [f[0, :, 4:4 + h, 12:12 + w].contiguous().to(dev) for f in smooth_frames("evalgop", 1, n, 128)]
    plain = evaluation.eval_gop(imodel, stem, frames, gop=12, with_msssim=False)
    path = tmp_path / "decoded.yuv"
    res = evaluation.eval_gop(imodel, stem, frames, gop=12, with_msssim=False, yuv=True, write_to=path)
    assert set(res) - set(plain) == {"psnr_y_ave", "psnr_u_ave", "psnr_v_ave", "psnr_yuv_ave"}
    seq = data.YUVSequence(path, w, h, device="cpu")
    assert len(seq) == n
    for t, (a, b) in enumerate(zip(plain["frames"], res["frames"])):
        assert set(b) - set(a) == {"psnr_y", "psnr_u", "psnr_v", "psnr_yuv"}
        assert a["strings"] == b["strings"] and a["bpp"] == b["bpp"] and a["psnr"] == b["psnr"] and a["type"] == b["type"]
        source = [p.cpu().numpy().astype(np.int64) for p in F.rgb_to_yuv420(frames[t].unsqueeze(0), bit_depth=8)]
        want = []
        for p, s, k in zip(seq.planes(t), source, ("psnr_y", "psnr_u", "psnr_v")):
            mse = float(((p.numpy().astype(np.int64) - s) ** 2).mean())
            assert mse > 0
            want.append(10 * math.log10(255.0 ** 2 / mse))
            assert abs(b[k] - want[-1]) <= 1e-9 * abs(want[-1]), (t, k, b[k], want[-1])
        assert abs(b["psnr_yuv"] - (6 * want[0] + want[1] + want[2]) / 8) <= 1e-9 * abs(b["psnr_yuv"])
    for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv"):
        assert abs(res[k + "_ave"] - np.mean([f[k] for f in res["frames"]])) <= 1e-12 * abs(res[k + "_ave"])
    # a frame measured against itself: no error at all is +inf
    same = evaluation._yuv_metrics(frames[0], frames[0].unsqueeze(0), True, None)
    assert same["psnr_y"] == same["psnr_u"] == same["psnr_v"] == same["psnr_yuv"] == float("inf")


def test_yuv_sequence_frames_carry_their_planes_into_eval(tmp_path, dev):
    """a 10-bit sequence: `_yuv_metrics` measures against the planes the frame carries, at the frame's bit depth"""
    from spatiotemporalentropymodel_amd import data, evaluation, functional as F
    h, w = 6, 10
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 1024, size=s).astype("<u2") for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    path = tmp_path / "src.yuv"
    path.write_bytes(b"".join(p.tobytes() for p in planes))
    (frame,) = list(data.YUVSequence(path, w, h, bit_depth=10, device=dev))
    x_hat = (frame * 0.5).unsqueeze(0)
    got = evaluation._yuv_metrics(frame, x_hat, True, None)
    q = [p.cpu().numpy().astype(np.int64) for p in F.rgb_to_yuv420(x_hat, bit_depth=10)]
    for k, a, s in zip(("psnr_y", "psnr_u", "psnr_v"), q, planes):
        want = 10 * math.log10(1023.0 ** 2 / float(((a[0] - s.astype(np.int64)) ** 2).mean()))
        assert abs(got[k] - want) <= 1e-9 * want
