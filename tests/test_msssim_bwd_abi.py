"""CPU: the C ABI of the MS-SSIM backward kernel (include/stem_hip.h: stem_ms_ssim_bwd, stem_ms_ssim_bwd_workspace) and the
argument checks of the Python surface on top of it (functional.ms_ssim_backward, losses.ms_ssim, RateDistortionLoss(metric=...)).
Argument errors are reported before anything touches a device, so all of this runs without one."""
import ctypes as C

import pytest
import torch


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def test_symbols_are_declared_and_exported():
    lib = _lib()
    assert {"stem_ms_ssim_bwd", "stem_ms_ssim_bwd_workspace"} <= set(lib.declared_hip_symbols())
    raw = C.CDLL(lib.HIP_SO)
    for name in ("stem_ms_ssim_bwd", "stem_ms_ssim_bwd_workspace"):
        assert getattr(raw, name) is not None
    assert lib.hip().stem_abi_version() == 5
    assert lib.hip().stem_tape_entry_recordable(C.cast(raw.stem_ms_ssim_bwd, C.c_void_p)) == 1


def test_workspace_size_needs_no_device():
    h = _lib().hip()
    n = C.c_size_t(0)
    assert h.stem_ms_ssim_bwd_workspace(1, 3, 1080, 1920, C.byref(n)) == 0
    one = n.value
    # the fp64 gradient planes of scales 2-5; under one fp64 copy of the input
    assert 3 * 8 * (540 * 960 + 270 * 480 + 135 * 240 + 68 * 120) <= one < 3 * 8 * 1080 * 1920
    assert h.stem_ms_ssim_bwd_workspace(8, 3, 1080, 1920, C.byref(n)) == 0 and 7 * one < n.value <= 8 * one
    assert h.stem_ms_ssim_bwd_workspace(1, 3, 161, 161, C.byref(n)) == 0 and n.value > 0
    for bad in ((1, 3, 1080, 1920, None), (1, 3, 160, 1920, C.byref(n)), (1, 3, 1080, 160, C.byref(n)), (1, 3, 100, 100, C.byref(n)),
                (0, 3, 256, 256, C.byref(n))):
        assert h.stem_ms_ssim_bwd_workspace(*bad) != 0 and b"stem_ms_ssim_bwd_workspace" in h.stem_last_error(), bad


def test_argument_errors_name_the_function():
    h = _lib().hip()
    nf, nb = C.c_size_t(0), C.c_size_t(0)
    assert h.stem_ms_ssim_workspace(1, 3, 256, 256, C.byref(nf)) == 0
    assert h.stem_ms_ssim_bwd_workspace(1, 3, 256, 256, C.byref(nb)) == 0
    p = 4096                                         # never dereferenced: every call below fails its argument checks first
    ok = dict(x=p, y=p, B=1, C=3, H=256, W=256, data_range=1.0, fwd=p, fwd_bytes=nf.value, grad_ms=p, ws=p, ws_bytes=nb.value, dx=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = h.stem_ms_ssim_bwd(a["x"], a["y"], a["B"], a["C"], a["H"], a["W"], a["data_range"], a["fwd"], a["fwd_bytes"], a["grad_ms"],
                                a["ws"], a["ws_bytes"], a["dx"], None)
        return rc, h.stem_last_error()

    for bad in (dict(x=None), dict(y=None), dict(fwd=None), dict(grad_ms=None), dict(ws=None), dict(dx=None),      # a null pointer
                dict(H=160), dict(W=160), dict(H=160, W=160),                                                     # no fifth scale
                dict(fwd_bytes=nf.value - 1), dict(fwd_bytes=0), dict(ws_bytes=nb.value - 1), dict(ws_bytes=0),   # a workspace too small
                dict(data_range=0.0), dict(data_range=-1.0), dict(B=0), dict(B=-2)):
        rc, msg = call(**bad)
        assert rc != 0 and b"stem_ms_ssim_bwd" in msg, (bad, rc, msg)
    assert b"fifth scale" in call(H=160)[1]
    assert b"forward workspace" in call(fwd_bytes=16)[1]
    assert b"stem_ms_ssim_bwd_workspace" in call(ws_bytes=16)[1]


def test_metric_is_checked_at_construction():
    from spatiotemporalentropymodel_amd.losses import RateDistortionLoss
    for bad in ("psnr", "msssim", "MSE", None):
        with pytest.raises(ValueError):
            RateDistortionLoss(metric=bad)
    assert RateDistortionLoss().metric == "mse" and RateDistortionLoss(lmbda=0.5).lmbda == 0.5
    assert RateDistortionLoss(metric="ms-ssim").metric == "ms-ssim"


@pytest.mark.parametrize("metric", ["mse", "ms-ssim"])
def test_criterion_has_no_cpu_route(metric):
    from spatiotemporalentropymodel_amd.losses import RateDistortionLoss
    x = torch.rand(1, 3, 192, 192)
    out = {"x_hat": x.clone().requires_grad_(True), "likelihoods": {"y": torch.rand(1, 4, 12, 12) * 0.9 + 0.05}}
    with pytest.raises(RuntimeError):
        RateDistortionLoss(metric=metric)(out, x)
    with pytest.raises(RuntimeError):
        RateDistortionLoss()(out, x)


def test_differentiable_ms_ssim_has_no_cpu_route():
    from spatiotemporalentropymodel_amd import functional as F, losses
    x = torch.rand(1, 3, 192, 192)
    with pytest.raises(RuntimeError):
        losses.ms_ssim(x.clone().requires_grad_(True), x)
    with pytest.raises(RuntimeError):
        losses.ms_ssim(x, x, data_range=255.0)
    with pytest.raises(RuntimeError):
        F.ms_ssim_backward(x, x, torch.ones(1))
