"""CPU suite for tests/train_tail_ref.py: the references that tests/test_hip_train_tail.py holds the HIP kernels to are pinned here
(known-answer vectors, torch in float64), and every precondition its gates rest on is checked on the reference alone."""
import math

import numpy as np
import pytest
import torch

import train_tail_ref as ref
from conftest import close_ratio


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("ctr, key, want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    """the Random123 known-answer vectors of philox4x32-10"""
    got = ref.philox4x32_10(np.array([_words(ctr)], np.uint64), _words(key))
    assert [int(w) for w in got[0]] == _words(want)


def test_philox_uniform_stream_layout():
    """value i = word i & 3 of block i >> 2; counter = offset + epoch * 2^40 + block, carried into the high word and wrapped at 2^64;
    the seed's high half is the second key word; fp32 values are exact multiples of 2^-24 in [-1/2, 1/2)"""
    seed, off = (0xA4093822 << 32) | 0x299F31D0, 2 ** 32 - 2
    r = ref.philox_uniform(13, seed, off)
    for q in range(4):
        c = off + q
        w = ref.philox4x32_10(np.array([[c & 0xFFFFFFFF, c >> 32, 0, 0]], np.uint64), [seed & 0xFFFFFFFF, seed >> 32])[0]
        want = ((w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 - 0.5)[:13 - 4 * q]
        assert np.array_equal(r[4 * q:4 * q + 4].astype(np.float64), want)
    assert r.dtype == np.float32 and r.min() >= -0.5 and r.max() < 0.5
    assert np.array_equal(ref.philox_uniform(8, seed, 2 ** 64 - 1)[4:], ref.philox_uniform(4, seed, 0))            # wraps
    assert np.array_equal(ref.philox_uniform(8, seed, 5, epoch=3), ref.philox_uniform(8, seed, 5 + 3 * 2 ** 40))
    assert not np.array_equal(ref.philox_uniform(8, seed, 0), ref.philox_uniform(8, seed & 0xFFFFFFFF, 0))
    big = ref.philox_uniform(1 << 16, 7, 0).astype(np.float64)
    assert abs(big.mean()) < 5e-3 and abs(big.var() - 1 / 12) < 2e-3


@pytest.mark.parametrize("name", [c[0] for c in ref.ADAM_CASES])
def test_adam_reference_matches_torch_float64(name):
    """adam_reference == clip_grad_norm_ + torch.optim.Adam in torch.float64 over three steps (to the rounding of float64)"""
    c = ref.adam_case(name)
    p0, grads = ref.adam_inputs()
    run = ref.adam_reference_run(name)
    tor = ref.adam_torch(p0, grads, ref.ADAM_LR, torch.float64, *ref.ADAM_BETAS, ref.ADAM_EPS, c["max_norm"], c["gscale"])
    for step, (r, (p, m, v)) in enumerate(zip(run, tor), 1):
        for what, a, b in (("m", r["m"], m), ("v", r["v"], v), ("dp", r["p"] - r["p_old"], p - r["p_old"])):
            nz = b != 0
            assert np.array_equal(a == 0, b == 0)
            # dp = p_new - p_old loses |p| / |dp| < 2^10 of float64's 2^-53; m, v: a handful of roundings
            assert close_ratio(a[nz], b[nz], 0.0) < 1e-12, (what, step)


def test_adam_case_preconditions():
    """What the Adam gates of tests/test_hip_train_tail.py assume, shown on the references alone:
      - the gradients span 1e-9 .. 1e+1 with exact zeros, and sqrt(v) / sqrt(bc2) crosses eps;
      - the "noclip" case stays below max_norm in every step, the "clip" cases above it, "nonorm" has max_norm = 0;
      - half an ulp of p (the absolute floor the update is granted) is below 1e-5 of |dp| wherever dp != 0;
      - torch's own fp32 run passes every gate (1e-4) with at least a factor 4 to spare."""
    p0, grads = ref.adam_inputs()
    g = np.abs(grads[0][grads[0] != 0])
    assert np.abs(p0).max() <= 2.0 ** -10 and g.min() < 2e-9 and g.max() > 5.0 and (grads[0] == 0).sum() >= 80
    assert ref.ADAM_N % 4096 % 256 != 0 and ref.ADAM_N > 2 * 4096
    for name, rel, gscale in ref.ADAM_CASES:
        c = ref.adam_case(name)
        run = ref.adam_reference_run(name)
        t32 = ref.adam_torch(p0, grads, ref.ADAM_LR, torch.float32, *ref.ADAM_BETAS, ref.ADAM_EPS, c["max_norm"], c["gscale"])
        for step, (r, gr, (p32, m32, v32)) in enumerate(zip(run, grads, t32), 1):
            norm = math.sqrt(math.fsum((gr.astype(np.float64) * gscale) ** 2))
            if rel == 0.0:
                assert c["max_norm"] == 0.0
            elif rel > 1:
                assert norm + 1e-6 < c["max_norm"] and np.array_equal(r["g_eff"], gr.astype(np.float64) * gscale)
            else:
                assert norm > 1.3 * c["max_norm"]
            nz = r["v"] != 0
            root = np.sqrt(r["v"][nz]) / math.sqrt(1 - ref.ADAM_BETAS[1] ** step)
            assert root.min() < 0.2 * ref.ADAM_EPS and root.max() > 1e6 * ref.ADAM_EPS      # both sides of eps, by a wide margin
            dp = (r["p"] - r["p_old"])[nz]
            p_old32 = r["p_old"].astype(np.float32) if step == 1 else t32[step - 2][0].astype(np.float32)
            atol = ref.half_ulp32(np.maximum(np.abs(r["p_old"]), np.abs(r["p"])).astype(np.float32))[nz]
            assert (atol < 1e-5 * np.abs(dp)).all(), (name, step, float((atol / np.abs(dp)).max()))
            # the yardstick: torch's fp32 trajectory (its own m, v, p of the step before) against the float64 trajectory
            for what, (a, b, at, fl) in ref.adam_ratios(r, p_old32, p32.astype(np.float32), m32, v32).items():
                ratio = close_ratio(a, b, fl, at)
                assert ratio <= 1e-4 / 4, (name, step, what, ratio)


def test_likelihood_references_in_double():
    """the float64 likelihoods are what the formulas say at points that can be checked by hand, and the fp32 run of the same code (the
    yardstick the gates print) is well inside the project's 1e-4"""
    out = np.array([[0.0, 0.3], [7.5, -2.0]], np.float32)
    sc = np.array([[1.0, 0.01], [1.0, 2.0]], np.float32)
    mu = np.array([[0.0, 0.3], [0.0, 1.0]], np.float32)
    lik = ref.gc_likelihood(out, sc, mu)
    phi = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))                  # noqa: E731
    assert abs(lik[0, 0] - (phi(0.5) - phi(-0.5))) < 1e-15
    assert abs(lik[0, 1] - (phi(0.5 / 0.11) - phi(-0.5 / 0.11))) < 1e-15  # the scale is raised to scale_bound
    assert lik[1, 0] == 1e-9                                              # floored
    assert abs(lik[1, 1] - (phi(-2.5 / 2) - phi(-3.5 / 2))) < 1e-15
    for (B, H, W, C) in ref.TAIL_SHAPES[:1]:
        y, noise, scales, means = ref.gc_inputs(B, H, W, C, 5, tie=True)
        o = y + noise
        l64, l32 = ref.gc_likelihood(o, scales, means), ref.gc_likelihood(o, scales, means, torch.float32)
        assert (l64 == 1e-9).sum() >= o.size // 20 and (scales < 0.11).mean() > 0.2 and (o == means).sum() >= o.size // 14
        assert close_ratio(l32, l64, 0.1, 1e-9) < 2.5e-5
        coef = -1.0 / (math.log(2.0) * B * H * W)
        ds, dm = ref.gc_backward(o, scales, means, coef)
        low = scales < 0.11
        assert (ds[low] <= 0).all() and (ds[low] < 0).any() and (ds[low] == 0).any()       # passes only where it pushes the scale up
        assert (dm[o == means] == 0).all() and np.isfinite(ds).all() and np.isfinite(dm).all()
        pack = ref.eb_random_pack(C, 3)
        z, zn = ref.eb_inputs(B, H, W, C, 4)
        e64, e32 = ref.eb_likelihood(z + zn, pack), ref.eb_likelihood(z + zn, pack, torch.float32)
        assert e64.min() == 1e-9 and (e64 == 1e-9).sum() >= z.size // 20 and 0.1 < e64.max() < 1.0
        assert close_ratio(e32, e64, 0.1, 1e-9) < 2.5e-5
        # a likelihood is the mass of [v - 1/2, v + 1/2): over consecutive integers it sums to 1
        grid = np.repeat(np.arange(-60, 61, dtype=np.float32)[:, None], C, axis=1)
        assert np.abs(ref.eb_likelihood(grid, pack).sum(0) - 1.0).max() < 1e-6
