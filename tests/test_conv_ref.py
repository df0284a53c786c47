"""CPU suite for tests/conv_ref.py: the float64 statements that tests/test_hip_fp32_plans.py holds the fp32-MFMA kernels to are
pinned here against the CPU oracle (oracle/stem_oracle.py: double accumulation, results rounded to fp32), every channel within
1e-5 of its own maximum, and against the golden vectors captured from the reference (tests/golden/ops_small.npz) at the gate
tests/test_oracle_vs_golden.py holds the oracle to (1e-5, floor 0.1).  No HIP code is touched."""
import os
import sys

import numpy as np
import pytest

import conv_ref as ref
from conftest import REPO, assert_close

sys.path.insert(0, os.path.join(REPO, "oracle"))
import stem_oracle as orc  # noqa: E402


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


def per_channel(a, b, what, axis=1, rtol=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    red = tuple(i for i in range(b.ndim) if i != axis)
    cmax, err = np.abs(b).max(axis=red), np.abs(a - b).max(axis=red)
    assert cmax.min() > 0, what
    assert (err <= rtol * cmax).all(), f"{what}: worst err / own max {float((err / cmax).max()):.2e}"


CONV = [  # B, C, H, W, K, R, stride, pad
    (1, 40, 9, 11, 200, 3, 1, 1),
    (2, 37, 13, 10, 70, 5, 2, 2),
    (3, 64, 12, 12, 192, 1, 1, 0),
    (1, 3, 17, 23, 64, 5, 2, 2),
    (2, 6, 8, 7, 5, 3, 2, 0),           # no padding, rows and columns the stride leaves over
]


@pytest.mark.parametrize("shape", CONV)
def test_conv_vs_oracle(shape):
    B, C, H, W, K, R, st, pd = shape
    x, w, b = rnd((B, C, H, W), 1), rnd((K, C, R, R), 2, -0.1, 0.1), rnd((K,), 3)
    y = orc.conv2d_fwd(x, w, b, st, pd)
    per_channel(ref.conv2d_fwd(x, w, b, st, pd), y, "y")
    dy = rnd(y.shape, 4)
    dx, dw, db = orc.conv2d_bwd(x, w, dy, st, pd)
    per_channel(ref.conv2d_dx(dy, w, x.shape, st, pd), dx, "dx")
    per_channel(ref.conv2d_dw(x, dy, R, R, st, pd), dw, "dw", axis=0)
    assert_close(ref.bias_grad(dy), db, 1e-5, what="db", floor=0.1)


@pytest.mark.parametrize("shape", [(2, 48, 5, 7, 100, 5, 2, 2, 1), (2, 64, 5, 7, 3, 5, 2, 2, 1), (1, 5, 4, 3, 6, 3, 1, 1, 0), (2, 4, 3, 5, 7, 4, 2, 1, 0)])
def test_deconv_vs_oracle(shape):
    B, C, H, W, K, R, st, pd, op = shape
    x, w, b = rnd((B, C, H, W), 11), rnd((C, K, R, R), 12, -0.1, 0.1), rnd((K,), 13)
    y = orc.deconv2d_fwd(x, w, b, st, pd, op)
    assert y.shape[2:] == ref.deconv_out_hw(H, W, R, R, st, pd, op)
    per_channel(ref.deconv2d_fwd(x, w, b, st, pd, op), y, "y")
    dy = rnd(y.shape, 14)
    dx, dw, db = orc.deconv2d_bwd(x, w, dy, st, pd, op)
    per_channel(ref.deconv2d_dx(dy, w, st, pd), dx, "dx")
    per_channel(ref.deconv2d_dw(x, dy, R, R, st, pd), dw, "dw", axis=1)
    assert_close(ref.bias_grad(dy), db, 1e-5, what="db", floor=0.1)


def test_mask_and_activations_vs_oracle():
    w = rnd((6, 4, 5, 5), 21)
    np.testing.assert_array_equal(w * ref.mask_a(5, 5), orc.masked_weight(w))
    assert ref.mask_a(5, 5).sum() == 12 and ref.mask_a(3, 3).sum() == 4 and ref.mask_a(1, 1).sum() == 0
    v, g = rnd((2, 5, 4, 3), 22), rnd((2, 5, 4, 3), 23)
    v[0, 0, 0, :2] = (0.0, -0.0)
    np.testing.assert_array_equal(ref.lrelu(v, np.float32(0.01)).astype(np.float32), orc.lrelu_fwd(v))
    np.testing.assert_array_equal(ref.dact(g, v, np.float32(0.01)).astype(np.float32), orc.lrelu_bwd(v, g))
    assert (ref.dact(g, v, 0.25)[0, 0, 0, :2] == 0.25 * g[0, 0, 0, :2].astype(np.float64)).all()        # 0.0 and -0.0 take the slope


def _gdn_operands(C, seed):
    x, dy = rnd((2, C, 5, 6), seed, -3, 3), rnd((2, C, 5, 6), seed + 1)
    beta = np.sqrt(1 + 0.2 * rnd((C,), seed + 2) + 2.0 ** -36).astype(np.float32)
    gamma = np.sqrt(0.1 * np.eye(C) + 0.02 * np.abs(rnd((C, C), seed + 3)) + 2.0 ** -36).astype(np.float32)
    gamma[1, :3] = 0.0                 # below 2^-18: the effective gamma is exactly 0
    gamma[2, 4] = 2.0 ** -19
    beta[3] = 0.0                      # below its bound
    return x, dy, beta, gamma


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_vs_oracle(inverse):
    x, dy, beta, gamma = _gdn_operands(12, 31)
    eb, eg = ref.gdn_params(beta, gamma)
    assert eg[1, 0] == 0.0 and eg[2, 4] == 0.0 and abs(eb[3] - 1e-6) < 1e-12
    per_channel(ref.gdn_fwd(x, beta, gamma, int(inverse)), orc.gdn_fwd(x, beta, gamma, inverse=inverse), "y")
    n = ref.gdn_fwd(x, beta, gamma, 2)
    np.testing.assert_allclose(x / np.sqrt(n), ref.gdn_fwd(x, beta, gamma, 0), rtol=1e-15)
    dx, db, dg = orc.gdn_bwd(x, dy, beta, gamma, inverse=inverse)
    rx, rb, rg = ref.gdn_bwd(x, dy, beta, gamma, inverse=inverse)
    per_channel(rx, dx, "dx")
    assert_close(rb, db, 1e-5, what="dbeta", floor=0.1)
    assert_close(rg, dg, 1e-5, what="dgamma", floor=0.1)
    assert (rg[1, :3] <= 0).all() and ((rg[1, :3] == 0) | (rg[1, :3] < 0)).all()     # below the bound: only upward pushes pass


def test_gdn_gamma_contraction_is_the_squared_operand_weight_gradient():
    """the contraction the gamma gradient runs on the weight-gradient kernel: a 1x1 weight gradient with x^2 as the gathered operand"""
    g, x = rnd((2, 8, 4, 5), 41), rnd((2, 8, 4, 5), 42, -3, 3)
    want = ref.conv2d_dw(x.astype(np.float64) ** 2, g, 1, 1, 1, 0)[:, :, 0, 0]
    np.testing.assert_allclose(ref.gdn_gamma_contraction(g, x), want, rtol=1e-13)


@pytest.mark.parametrize("name", ["conv_k5s2", "conv_k5s1", "conv_k3s1", "conv_k1s1", "conv_c3"])
def test_conv_golden(golden, name):
    g = golden("ops_small.npz")
    N, C, H, W, K, R, st, pd = (int(v) for v in g[f"{name}:cfg"])
    x, w, b, dy = g[f"{name}:x"], g[f"{name}:w"], g[f"{name}:b"], g[f"{name}:dy"]
    assert_close(ref.conv2d_fwd(x, w, b, st, pd), g[f"{name}:y"], 1e-5, what=name + " y", floor=0.1)
    assert_close(ref.conv2d_dx(dy, w, x.shape, st, pd), g[f"{name}:dx"], 1e-5, what=name + " dx", floor=0.1)
    assert_close(ref.conv2d_dw(x, dy, R, R, st, pd), g[f"{name}:dw"], 1e-5, what=name + " dw", floor=0.1)
    assert_close(ref.bias_grad(dy), g[f"{name}:db"], 1e-5, what=name + " db", floor=0.1)


@pytest.mark.parametrize("name", ["deconv_k5s2", "deconv_c3"])
def test_deconv_golden(golden, name):
    g = golden("ops_small.npz")
    N, C, H, W, K, R, st, pd, op = (int(v) for v in g[f"{name}:cfg"])
    x, w, b, dy = g[f"{name}:x"], g[f"{name}:w"], g[f"{name}:b"], g[f"{name}:dy"]
    assert_close(ref.deconv2d_fwd(x, w, b, st, pd, op), g[f"{name}:y"], 1e-5, what=name + " y", floor=0.1)
    assert_close(ref.deconv2d_dx(dy, w, st, pd), g[f"{name}:dx"], 1e-5, what=name + " dx", floor=0.1)
    assert_close(ref.deconv2d_dw(x, dy, R, R, st, pd), g[f"{name}:dw"], 1e-5, what=name + " dw", floor=0.1)
    assert_close(ref.bias_grad(dy), g[f"{name}:db"], 1e-5, what=name + " db", floor=0.1)


def test_masked_conv_golden(golden):
    g = golden("ops_small.npz")
    n = "masked_k5"
    wm = g[f"{n}:w_before"] * ref.mask_a(5, 5)
    np.testing.assert_array_equal(wm.astype(np.float32), g[f"{n}:w_after"])
    assert_close(ref.conv2d_fwd(g[f"{n}:x"], wm, g[f"{n}:b"], 1, 2), g[f"{n}:y"], 1e-5, what="masked y", floor=0.1)
    assert_close(ref.conv2d_dx(g[f"{n}:dy"], wm, g[f"{n}:x"].shape, 1, 2), g[f"{n}:dx"], 1e-5, what="masked dx", floor=0.1)
    assert_close(ref.conv2d_dw(g[f"{n}:x"], g[f"{n}:dy"], 5, 5, 1, 2), g[f"{n}:dw"], 1e-5, what="masked dw (all 25 taps)", floor=0.1)


def test_gdn_golden(golden):
    g = golden("ops_small.npz")
    for n, inv in (("gdn", False), ("igdn", True)):
        x, dy, beta, gamma = g[f"{n}:x"], g[f"{n}:dy"], g[f"{n}:beta"], g[f"{n}:gamma"]
        assert_close(ref.gdn_fwd(x, beta, gamma, int(inv)), g[f"{n}:y"], 1e-5, what=n, floor=0.1)
        dx, db, dg = ref.gdn_bwd(x, dy, beta, gamma, inverse=inv)
        assert_close(dx, g[f"{n}:dx"], 1e-5, what=n + " dx", floor=0.1)
        assert_close(db, g[f"{n}:dbeta"], 1e-5, what=n + " dbeta", floor=0.1)
        assert_close(dg, g[f"{n}:dgamma"], 1e-5, what=n + " dgamma", floor=0.1)
    x = g["gdn_init:x"]
    assert_close(ref.gdn_fwd(x, g["gdn_init:beta"], g["gdn_init:gamma"]), x / np.sqrt(1 + 0.1 * x.astype(np.float64) ** 2), 1e-5,
                 what="gdn closed form", floor=0.1)
