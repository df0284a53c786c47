"""CPU: the C ABI of the YUV 4:2:0 kernels (include/stem_hip.h: stem_yuv420_to_rgb, stem_rgb_to_yuv420, stem_rgb_to_yuv420_workspace),
the host side of transforms / data.YUVSequence / write_yuv420, and the new keywords of evaluation.  Argument errors are reported
before anything touches a device, so all of this runs without one."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

NAMES = ("stem_yuv420_to_rgb", "stem_rgb_to_yuv420", "stem_rgb_to_yuv420_workspace", "stem_ycbcr_convert", "stem_plane_resample2")


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def fx():
    import yuv_fixture
    return yuv_fixture, yuv_fixture.load()


def test_symbols_are_declared_and_exported():
    lib = _lib()
    assert set(NAMES) <= set(lib.declared_hip_symbols())
    raw = C.CDLL(lib.HIP_SO)
    for name in NAMES:
        assert getattr(raw, name) is not None
    assert lib.hip().stem_abi_version() == 5


def test_workspace_size_needs_no_device():
    h = _lib().hip()
    n = C.c_size_t(0)
    assert h.stem_rgb_to_yuv420_workspace(1, 1080, 1920, C.byref(n)) == 0
    one = n.value
    # three 64-bit slots per workgroup of 256 work items of 2 x 4 pixels
    assert one == 24 * -(-(540 * 480) // 256)
    assert h.stem_rgb_to_yuv420_workspace(16, 1080, 1920, C.byref(n)) == 0 and n.value == 16 * one
    assert h.stem_rgb_to_yuv420_workspace(1, 2, 2, C.byref(n)) == 0 and n.value == 24
    for bad in ((1, 1080, 1920, None), (0, 2, 2, C.byref(n)), (1, 3, 2, C.byref(n)), (1, 2, 0, C.byref(n))):
        assert h.stem_rgb_to_yuv420_workspace(*bad) != 0 and b"stem_rgb_to_yuv420_workspace" in h.stem_last_error(), bad


def test_yuv420_to_rgb_argument_errors_name_the_function():
    h = _lib().hip()
    p = 4096                                         # never dereferenced: every call below fails its argument checks first
    ok = dict(y=p, u=p, v=p, B=1, H=4, W=6, sb=1, bd=8, up=0, clamp=1, rgb=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = h.stem_yuv420_to_rgb(a["y"], a["u"], a["v"], a["B"], a["H"], a["W"], a["sb"], a["bd"], a["up"], a["clamp"], a["rgb"], None)
        return rc, h.stem_last_error()

    for bad in (dict(y=None), dict(u=None), dict(v=None), dict(rgb=None),                 # a null pointer
                dict(H=5), dict(W=7), dict(H=0), dict(W=0), dict(H=-2),                    # odd or empty sides
                dict(bd=9), dict(bd=10), dict(sb=2, bd=9), dict(sb=2, bd=12), dict(sb=4), dict(sb=0),
                dict(B=0), dict(B=-1), dict(up=2), dict(up=-1),
                dict(sb=2, bd=10, y=p + 1)):                                               # a 16-bit plane on an odd address
        rc, msg = call(**bad)
        assert rc != 0 and b"stem_yuv420_to_rgb" in msg, (bad, rc, msg)
    assert b"even" in call(H=5)[1] and b"bit_depth" in call(bd=9)[1]


def test_rgb_to_yuv420_argument_errors_name_the_function():
    h = _lib().hip()
    n = C.c_size_t(0)
    assert h.stem_rgb_to_yuv420_workspace(2, 34, 70, C.byref(n)) == 0
    p = 4096
    ok = dict(rgb=p, B=2, H=34, W=70, yf=None, uf=None, vf=None, yi=p, ui=p, vi=p, sb=1, bd=8, ys=p, us=p, vs=p, ws=p, wsb=n.value, sse=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = h.stem_rgb_to_yuv420(a["rgb"], a["B"], a["H"], a["W"], a["yf"], a["uf"], a["vf"], a["yi"], a["ui"], a["vi"], a["sb"], a["bd"],
                                  a["ys"], a["us"], a["vs"], a["ws"], a["wsb"], a["sse"], None)
        return rc, h.stem_last_error()

    for bad in (dict(rgb=None), dict(yi=None), dict(ui=None), dict(vs=None), dict(sse=None), dict(ws=None),          # null pointers
                dict(yi=None, ui=None, vi=None),                                     # squared errors without integer planes, no output
                dict(yf=p), dict(yf=p, uf=p),                                        # an incomplete set of fp32 planes
                dict(ys=None, us=None, vs=None),                                     # sums without source planes
                dict(H=33), dict(W=71), dict(H=0), dict(bd=9), dict(bd=10), dict(sb=3), dict(B=0),
                dict(wsb=n.value - 1), dict(wsb=0),                                  # workspace too small
                dict(ws=p + 4), dict(sse=p + 4)):                                    # 64-bit slots on a 4-byte boundary
        rc, msg = call(**bad)
        assert rc != 0 and b"stem_rgb_to_yuv420" in msg, (bad, rc, msg)
    assert b"workspace" in call(wsb=8)[1] and b"bit_depth" in call(bd=9)[1]
    # fp32 planes alone need neither a sample format nor a workspace: only the geometry is checked
    rc, msg = call(yf=p, uf=p, vf=p, yi=None, ui=None, vi=None, ys=None, us=None, vs=None, sse=None, ws=None, wsb=0, sb=0, bd=0, H=33)
    assert rc != 0 and b"even" in msg


def test_single_step_argument_errors_name_the_function():
    h = _lib().hip()
    p = 4096
    for bad in ((None, p, 1, 4, 6, 0), (p, None, 1, 4, 6, 1), (p, p, 0, 4, 6, 0), (p, p, 1, 0, 6, 0), (p, p, 1, 4, -1, 1)):
        assert h.stem_ycbcr_convert(*bad, None) != 0 and b"stem_ycbcr_convert" in h.stem_last_error(), bad
    for bad in ((None, p, 1, 4, 6, 0), (p, None, 1, 4, 6, 2), (p, p, 0, 4, 6, 0), (p, p, 1, 0, 6, 1), (p, p, 1, 4, 6, 3), (p, p, 1, 4, 6, -1),
                (p, p, 1, 5, 6, 2), (p, p, 1, 4, 7, 2)):
        assert h.stem_plane_resample2(*bad, None) != 0 and b"stem_plane_resample2" in h.stem_last_error(), bad


def test_functional_has_no_cpu_route():
    from spatiotemporalentropymodel_amd import functional as F
    y, u = torch.zeros(1, 4, 6, dtype=torch.uint8), torch.zeros(1, 2, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        F.yuv420_to_rgb(y, u, u)
    with pytest.raises(RuntimeError):
        F.rgb_to_yuv420(torch.rand(1, 3, 4, 6))
    with pytest.raises(RuntimeError):
        F.rgb_to_yuv420(torch.rand(1, 3, 4, 6), bit_depth=8, source=(y, u, u))
    with pytest.raises(RuntimeError):
        F.ycbcr_convert(torch.rand(1, 3, 4, 6), True)
    with pytest.raises(RuntimeError):
        F.plane_resample2(torch.rand(1, 4, 6), 0)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_transforms_on_cpu_tensors_match_the_reference(fx):
    """transforms.* on host tensors against the reference's float32 arrays: 0 ulp, compared as bit patterns.  The module issues
    the reference's torch operations in the reference's order on the same inputs, and torch's CPU kernels round each of them
    identically from run to run, so nothing may move; a reordered formula or another interpolation order shows as 1 ulp.
    The class forms are held to the same arrays -- YUV420To444(mode="nearest") to the NEAREST ones: the constructor's mode is the
    mode used (the documented difference from the reference, whose class always interpolates bilinearly)."""
    from spatiotemporalentropymodel_amd import transforms as T
    mod, g = fx
    checked = 0
    for case, bits in mod.cases(g):
        if f"{case}/rgb32_bilinear" not in g:              # float32 results are kept for the shapes up to 34x70
            continue
        checked += 1
        peak, ref = float((1 << bits) - 1), g[f"{case}/ref_images"]
        planes = tuple(torch.from_numpy(g[f"{case}/{n}"][ref].astype(np.float32)).unsqueeze(1) / peak for n in "yuv")
        ints = tuple(torch.from_numpy(g[f"{case}/{n}"][ref]) for n in "yuv")
        for mode in ("bilinear", "nearest"):
            want = g[f"{case}/rgb32_{mode}"]
            assert _same_bits(T.ycbcr2rgb(T.yuv_420_to_444(planes, mode=mode)).numpy(), want), (case, mode)
            assert _same_bits(T.YCbCr2RGB()(T.YUV420To444(mode=mode)(planes)).numpy(), want), (case, mode)
            assert _same_bits(T.yuv420_planes_to_rgb(ints, bits, mode).numpy(), want), (case, mode)
        src = torch.from_numpy(g[f"{case}/src"][ref])
        for got in (T.yuv_444_to_420(T.rgb2ycbcr(src)), T.YUV444To420()(T.RGB2YCbCr()(src)), T.rgb_to_yuv420_planes(src)):
            for n, p in zip("yuv", got):
                assert _same_bits(p.reshape(g[f"{case}/{n}32"].shape).numpy(), g[f"{case}/{n}32"]), (case, n)
        for n, p in zip("yuv", T.rgb_to_yuv420_planes(src, bits)):
            want = mod.quantise(g[f"{case}/{n}32"], peak)
            assert p.dtype == (torch.uint8 if bits == 8 else torch.uint16) and np.array_equal(p.numpy().astype(np.float64), want), (case, n)
    assert checked >= 6                                    # 2x2, 4x6, 34x70 at both depths
    y, u, v = T.yuv_420_to_444(planes, return_tuple=True)
    assert y.shape == u.shape == v.shape
    assert T.rgb2ycbcr(src[0]).shape == src[0].shape                  # 3-D input


def test_transforms_raise_what_the_reference_raises():
    from spatiotemporalentropymodel_amd import transforms as T
    y, u = torch.rand(1, 1, 4, 4), torch.rand(1, 1, 2, 2)
    with pytest.raises(ValueError, match="Invalid upsampling mode"):
        T.yuv_420_to_444((y, u, u), mode="bicubic")
    with pytest.raises(ValueError, match="Invalid downsampling mode"):
        T.yuv_444_to_420(torch.rand(1, 3, 4, 4), mode="nearest")
    with pytest.raises(ValueError, match="tuple of 3"):
        T.yuv_420_to_444((y, u))
    with pytest.raises(ValueError, match="tuple of 3"):
        T.yuv_420_to_444((y, u, None))
    for bad in (torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.rand(1, 2, 4, 4), torch.rand(4, 4), [[0.0]]):
        with pytest.raises(ValueError, match="3D or 4D tensor"):
            T.rgb2ycbcr(bad)
        with pytest.raises(ValueError, match="3D or 4D tensor"):
            T.ycbcr2rgb(bad)
    assert repr(T.YUV420To444(return_tuple=True)) == "YUV420To444(return_tuple=True)" and repr(T.RGB2YCbCr()) == "RGB2YCbCr()"
    assert T.YUV420To444(mode="nearest").mode == "nearest" and T.YUV420To444("nearest", True).return_tuple is True
    assert T.YUV444To420().mode == "avg_pool"
    with pytest.raises(TypeError):
        T.RGB2YCbCr(mode="x")
    with pytest.raises(ValueError, match="Invalid downsampling mode"):
        T.YUV444To420(mode="nearest")(torch.rand(1, 3, 4, 4))


@pytest.mark.parametrize("bits", [8, 10])
def test_yuv_sequence_reads_files_on_the_host(tmp_path, bits):
    from spatiotemporalentropymodel_amd import data, transforms as T
    w, h, n = 10, 6, 3
    rng = np.random.default_rng(bits)
    dt = np.uint8 if bits == 8 else "<u2"
    frames = [[rng.integers(0, 1 << bits, size=s).astype(dt) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))] for _ in range(n)]
    path = tmp_path / "seq.yuv"
    with open(path, "wb") as f:
        for fr in frames:
            for p in fr:
                f.write(p.tobytes())
    seq = data.YUVSequence(path, w, h, bit_depth=bits, device="cpu")
    assert len(seq) == n and len(data.YUVSequence(path, w, h, bit_depth=bits, frames=2, device="cpu")) == 2
    for i, fr in enumerate(frames):
        got = seq.planes(i)
        assert [tuple(p.shape) for p in got] == [(1, h, w), (1, h // 2, w // 2), (1, h // 2, w // 2)]
        for p, want in zip(got, fr):
            assert p.dtype == (torch.uint8 if bits == 8 else torch.uint16) and np.array_equal(p[0].numpy(), want)
    out = list(seq)                                                     # device="cpu": the torch composition, planes attached
    assert len(out) == n and out[1].shape == (3, h, w) and out[1].bit_depth == bits
    assert all(np.array_equal(p[0].numpy(), want) for p, want in zip(out[1].yuv_planes, frames[1]))
    assert torch.equal(out[1], T.yuv420_planes_to_rgb(seq.planes(1), bits, "bilinear", True)[0])
    assert float(out[1].min()) >= 0.0 and float(out[1].max()) <= 1.0
    # a file that is not a whole number of frames, no frames at all, more frames than there are, odd geometry, a depth nobody ships
    with open(path, "ab") as f:
        f.write(b"\0" * 5)
    for bad in (dict(path=path), dict(path=path, frames=n + 1)):
        with pytest.raises(ValueError):
            data.YUVSequence(bad["path"], w, h, bit_depth=bits, frames=bad.get("frames"), device="cpu")
    empty = tmp_path / "empty.yuv"
    empty.write_bytes(b"")
    for args in ((empty, w, h, bits), (path, w + 1, h, bits), (path, w, h, 9)):
        with pytest.raises(ValueError):
            data.YUVSequence(args[0], args[1], args[2], bit_depth=args[3], device="cpu")


@pytest.mark.parametrize("bits", [8, 10])
def test_write_yuv420_of_host_frames_reads_back(tmp_path, bits):
    from spatiotemporalentropymodel_amd import data, transforms as T
    x = torch.rand(2, 3, 6, 10)
    path = tmp_path / "out.yuv"
    planes = data.write_yuv420(path, x, bit_depth=bits, append=False)
    data.write_yuv420(path, x[1], bit_depth=bits)                      # appends a third frame
    seq = data.YUVSequence(path, 10, 6, bit_depth=bits, device="cpu")
    assert len(seq) == 3
    want = T.rgb_to_yuv420_planes(x, bits)
    for i, b in enumerate((0, 1, 1)):
        for p, q, r in zip(seq.planes(i), planes, want):
            assert torch.equal(p[0], q[b]) and torch.equal(p[0], r[b])


def test_evaluation_keywords_default_to_off():
    from spatiotemporalentropymodel_amd import evaluation
    for fn in (evaluation.inference_iframe, evaluation.inference_pframe, evaluation.eval_gop):
        sig = inspect.signature(fn)
        assert sig.parameters["yuv"].default is False and sig.parameters["write_to"].default is None, fn.__name__

    seen = []

    def fake(model, x, with_msssim=True, **kw):
        seen.append(kw)
        return {"y_conditioned": None, "psnr": 1.0, "ms-ssim": None, "bpp": 1.0, "estimate_bpp": 1.0}

    orig = evaluation.inference_iframe
    evaluation.inference_iframe = fake
    try:
        res = evaluation.eval_gop(None, None, [torch.zeros(3, 2, 2)] * 2, all_intra=True)
    finally:
        evaluation.inference_iframe = orig
    assert seen == [{}, {}]                                              # nothing new is passed through
    assert set(res) == {"frames", "psnr_ave", "bpp_ave", "msssim_ave", "estimate_bpp_ave"}
    assert evaluation._yuv_metrics(torch.zeros(3, 2, 2), torch.zeros(1, 3, 2, 2), False, None) == {}
    assert evaluation._psnr_int(0, 10, 255) == float("inf")
    assert abs(evaluation._psnr_int(10, 10, 255) - 20 * np.log10(255)) < 1e-12
