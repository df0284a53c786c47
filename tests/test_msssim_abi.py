"""CPU: the C ABI of the MS-SSIM kernel (include/stem_hip.h: stem_ms_ssim, stem_ms_ssim_workspace).  Argument errors are reported
before anything touches a device, so all of this runs without one."""
import ctypes as C

import pytest
import torch


def _lib():
    from spatiotemporalentropymodel_amd import _lib
    return _lib


def test_symbols_are_declared_and_exported():
    lib = _lib()
    assert {"stem_ms_ssim", "stem_ms_ssim_workspace"} <= set(lib.declared_hip_symbols())
    raw = C.CDLL(lib.HIP_SO)
    for name in ("stem_ms_ssim", "stem_ms_ssim_workspace"):
        assert getattr(raw, name) is not None
    assert lib.hip().stem_abi_version() == 5


def test_workspace_size_needs_no_device():
    h = _lib().hip()
    n = C.c_size_t(0)
    assert h.stem_ms_ssim_workspace(1, 3, 1080, 1920, C.byref(n)) == 0
    one = n.value
    # at least the pooled planes of scales 2-5 of both images; well under two copies of the inputs
    assert 2 * 3 * 4 * (540 * 960 + 270 * 480 + 135 * 240 + 68 * 120) <= one < 2 * 3 * 4 * 1080 * 1920
    assert h.stem_ms_ssim_workspace(8, 3, 1080, 1920, C.byref(n)) == 0 and 7 * one < n.value <= 8 * one
    assert h.stem_ms_ssim_workspace(1, 3, 161, 161, C.byref(n)) == 0 and n.value > 0
    assert h.stem_ms_ssim_workspace(1, 3, 1080, 1920, None) != 0 and b"stem_ms_ssim_workspace" in h.stem_last_error()
    assert h.stem_ms_ssim_workspace(1, 3, 160, 1920, C.byref(n)) != 0 and b"stem_ms_ssim_workspace" in h.stem_last_error()


def test_argument_errors_name_the_function():
    h = _lib().hip()
    n = C.c_size_t(0)
    assert h.stem_ms_ssim_workspace(1, 3, 256, 256, C.byref(n)) == 0
    p = 4096                                         # never dereferenced: every call below fails its argument checks first
    ok = dict(x=p, y=p, B=1, C=3, H=256, W=256, data_range=1.0, workspace=p, workspace_bytes=n.value, ms_ssim=p, mse=None, terms=None)

    def call(**kw):
        a = dict(ok, **kw)
        rc = h.stem_ms_ssim(a["x"], a["y"], a["B"], a["C"], a["H"], a["W"], a["data_range"], a["workspace"], a["workspace_bytes"], a["ms_ssim"],
                            a["mse"], a["terms"], None)
        return rc, h.stem_last_error()

    for bad in (dict(x=None), dict(y=None), dict(workspace=None), dict(ms_ssim=None),        # a null pointer
                dict(H=160), dict(W=160), dict(H=160, W=160),                                 # no fifth scale
                dict(workspace_bytes=n.value - 1), dict(workspace_bytes=0),                   # workspace too small
                dict(data_range=0.0), dict(data_range=-1.0), dict(B=0)):
        rc, msg = call(**bad)
        assert rc != 0 and b"stem_ms_ssim" in msg, (bad, rc, msg)
    rc, msg = call(H=160)
    assert b"fifth scale" in msg
    rc, msg = call(workspace_bytes=16)
    assert b"workspace" in msg


def test_functional_has_no_cpu_route():
    from spatiotemporalentropymodel_amd import functional as F
    x = torch.rand(1, 3, 192, 192)
    with pytest.raises(RuntimeError):
        F.ms_ssim(x, x)
    with pytest.raises(RuntimeError):
        F.ms_ssim(x, x, return_terms=True)


def test_with_msssim_takes_only_device_as_a_string():
    from spatiotemporalentropymodel_amd import evaluation
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(ValueError):
        evaluation._metrics(x, x, "host")
    assert evaluation._metrics(x, x * 0.5, False)[1] is None
