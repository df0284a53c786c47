"""CPU: the numpy references of tests/cheng_ref.py pinned against independent statements -- the shuffle against
torch.nn.functional.pixel_shuffle and its autograd, add_act and the gate against float64 (and torch's autograd of the formulas)."""
import numpy as np
import pytest
import torch

import cheng_ref as R


def _rand(seed, shape, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("C", [3, 4, 36])
@pytest.mark.parametrize("slope", [1.0, 0.01])
def test_pixel_shuffle_matches_torch(r, C, slope):
    B, H, W = 2, 3, 5
    x = _rand(r * 100 + C, (B, H, W, C * r * r))
    add = _rand(7, (B, H * r, W * r, C))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).clone().requires_grad_(True)             # NCHW
    at = torch.from_numpy(add).permute(0, 3, 1, 2)
    y0 = torch.nn.functional.leaky_relu(torch.nn.functional.pixel_shuffle(xt, r), slope)
    yt = y0 + at
    # the blocks apply the activation AFTER the shuffle, the kernel before: the same thing element by element
    assert np.array_equal(R.pixel_shuffle_fwd(x, r, slope), y0.detach().permute(0, 2, 3, 1).numpy())
    assert np.array_equal(R.pixel_shuffle_fwd(x, r, slope, add), yt.detach().permute(0, 2, 3, 1).numpy())
    g = _rand(9, (B, H * r, W * r, C))
    yt.backward(torch.from_numpy(g).permute(0, 3, 1, 2))
    assert np.array_equal(R.pixel_shuffle_bwd(g, r, x, slope), xt.grad.permute(0, 2, 3, 1).numpy())
    if slope == 1.0:
        assert np.array_equal(R.pixel_shuffle_bwd(g, r), xt.grad.permute(0, 2, 3, 1).numpy())


def test_pixel_shuffle_is_a_permutation_and_its_backward_the_inverse():
    for r, C, shape in ((2, 3, (1, 7, 33)), (3, 8, (2, 3, 5)), (1, 4, (1, 1, 1))):
        x = np.arange(np.prod(shape) * C * r * r, dtype=np.float32).reshape(*shape, C * r * r) + 1.0
        y = R.pixel_shuffle_fwd(x, r)
        assert y.shape == (shape[0], shape[1] * r, shape[2] * r, C) and np.array_equal(np.sort(y.ravel()), np.sort(x.ravel()))
        assert np.array_equal(R.pixel_shuffle_bwd(y, r), x)
        b, h, w, c, i, j = 0, shape[1] - 1, shape[2] - 1, C - 1, r - 1, 0
        assert y[b, h * r + i, w * r + j, c] == x[b, h, w, c * r * r + i * r + j]


@pytest.mark.parametrize("slope", [0.0, 0.01])
def test_add_act_against_float64_and_autograd(slope):
    a, b = _rand(1, (2, 5, 7, 12)), _rand(2, (2, 5, 7, 12))
    a[0, 0, 0, :4], b[0, 0, 0, :4] = [0.5, -0.5, 0.0, 1.0], [-0.5, 0.5, 0.0, -1.0]          # exact zeros after the sum
    out = R.add_act_fwd(a, b, slope)
    s64 = a.astype(np.float64) + b.astype(np.float64)
    exact = np.where(s64 > 0, s64, s64 * slope)
    assert np.all(np.abs(out - exact) <= 2.0 ** -23 * np.abs(exact))
    assert np.all(out[0, 0, 0, :4] == 0)
    g = _rand(3, a.shape)
    at, bt = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    torch.nn.functional.leaky_relu(at + bt, slope).backward(torch.from_numpy(g))
    ours = R.add_act_bwd(out, g, slope)
    assert np.array_equal(ours, at.grad.numpy()) and np.array_equal(ours, bt.grad.numpy())
    assert np.array_equal(ours[0, 0, 0, :4], g[0, 0, 0, :4] * np.float32(slope))           # out == 0 takes the slope side


def _gate_inputs():
    a, x, g = _rand(4, (2, 6, 10, 24), -2, 2), _rand(5, (2, 6, 10, 24), -2, 2), _rand(6, (2, 6, 10, 24))
    b = _rand(8, (2, 6, 10, 24), -30, 30)
    b[0, 0, 0, :6] = [30.0, -30.0, 0.0, -0.0, 88.0, -88.0]
    return a, b, x, g


def test_gate_fp32_reference_is_inside_the_derived_bound():
    a, b, x, g = _gate_inputs()
    exact = R.gate_fwd(a, b, x, np.float64)
    assert np.allclose(exact, a.astype(np.float64) * (1 / (1 + np.exp(-b.astype(np.float64)))) + x, rtol=1e-14, atol=0)
    err = np.abs(R.gate_fwd(a, b, x).astype(np.float64) - exact)
    bound = R.gate_fwd_bound(a, b, x)
    assert np.all(err <= bound) and np.all(bound <= 8 * R.U * (np.abs(a) + np.abs(x)) + R.GATE_FLOOR)
    da, db = R.gate_bwd(a, b, g)
    da64, db64 = R.gate_bwd(a, b, g, np.float64)
    bda, bdb = R.gate_bwd_bounds(a, b, g)
    assert np.all(np.abs(da - da64) <= bda) and np.all(np.abs(db - db64) <= bdb)
    assert np.all(np.isfinite(db)) and np.all(np.isfinite(da))


def test_gate_backward_is_the_gradient_of_the_forward():
    a, b, x, g = _gate_inputs()
    ts = [torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in (a, b, x)]
    (ts[0] * torch.sigmoid(ts[1]) + ts[2]).backward(torch.from_numpy(g.astype(np.float64)))
    da64, db64 = R.gate_bwd(a, b, g, np.float64)
    assert np.allclose(da64, ts[0].grad.numpy(), rtol=1e-12, atol=1e-300)
    # torch forms 1 - s by subtraction: where s is close to 1 its gradient carries an absolute error of an ulp of 1, times |dout a|
    assert np.all(np.abs(db64 - ts[1].grad.numpy()) <= 1e-12 * np.abs(db64) + 2.0 ** -51 * np.abs(g.astype(np.float64) * a))
    assert np.array_equal(ts[2].grad.numpy(), g.astype(np.float64))
