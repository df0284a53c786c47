"""Float64 references for the tail of the training step: noise stream, likelihoods, loss reductions, norm, clip and Adam.

No GPU and nothing of the package's native code: tests/test_train_tail_ref.py pins these functions on the CPU (known-answer vectors,
torch.optim.Adam in float64), tests/test_hip_train_tail.py compares the HIP kernels with them.

  philox4x32_10 / philox_uniform   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) from the algorithm:
                                   counter (ctr_lo, ctr_hi, 0, 0), key (seed_lo, seed_hi), word -> (w >> 8) * 2^-24 - 0.5
  adam_reference                   torch.nn.utils.clip_grad_norm_ followed by the torch.optim.Adam single-tensor update
  eb_likelihood / gc_likelihood /  EntropyBottleneck / GaussianConditional (entropy_models.py:388-452, 570-596) through
  gc_backward                      oracle/stem_torch_cpu.py in torch.float64 (or float32: the yardstick the gates print)
  adam_case / adam_inputs          the inputs of the Adam parity case, with the preconditions its gates rest on
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "oracle"))

M32 = np.uint64(0xFFFFFFFF)
NOISE_EPOCH_STRIDE = 1 << 40


# ---------------------------------------------------------------------------------------------------------------- Philox4x32-10
def philox4x32_10(ctr, key):
    """ctr [n,4], key [n,2] or [2] (uint32 values) -> [n,4] uint32: ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped by the Weyl constants
    between rounds."""
    c = [np.asarray(ctr, np.uint64)[:, i] & M32 for i in range(4)]
    key = np.broadcast_to(np.asarray(key, np.uint64), (len(c[0]), 2))
    k0, k1 = key[:, 0] & M32, key[:, 1] & M32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for r in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & M32, (p0 >> s32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return np.stack(c, axis=1).astype(np.uint32)


def philox_uniform(n, seed, offset, epoch=0):
    """the n first values of the stream (seed, offset [+ epoch * 2^40]) as fp32 in [-0.5, 0.5): value i is word i & 3 of the block
    with the 64-bit counter offset + epoch * 2^40 + (i >> 2) (mod 2^64).  (w >> 8) * 2^-24 - 0.5 is exact in fp32: a multiple of
    2^-24 of magnitude at most 1/2."""
    nq = (n + 3) // 4
    base = (int(offset) + int(epoch) * NOISE_EPOCH_STRIDE) % (1 << 64)
    ctr = [(base + q) % (1 << 64) for q in range(nq)]
    ctr4 = np.zeros((nq, 4), np.uint64)
    ctr4[:, 0] = np.array([c & 0xFFFFFFFF for c in ctr], np.uint64)
    ctr4[:, 1] = np.array([c >> 32 for c in ctr], np.uint64)
    seed = int(seed) % (1 << 64)
    words = philox4x32_10(ctr4, [seed & 0xFFFFFFFF, seed >> 32]).reshape(-1)[:n]
    return ((words >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 - 0.5).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- clip + Adam
def clip_coef(g, max_norm, gscale=1.0):
    """the factor applied to g: gscale, times clip_grad_norm_'s min(1, max_norm / (|gscale g| + 1e-6)) when max_norm > 0"""
    if not max_norm > 0:
        return float(gscale)
    total = math.sqrt(math.fsum((np.asarray(g, np.float64) * gscale) ** 2))
    return float(gscale) * min(1.0, max_norm / (total + 1e-6))


def adam_reference(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, gscale=1.0):
    """-> (p, m, v, g_eff) after one step, float64: g_eff = g * gscale, clipped to max_norm (clip_grad_norm_, none for max_norm <= 0);
    then torch.optim.Adam's single-tensor update without amsgrad or weight decay:
    m.lerp_(g, 1 - b1); v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    g = g * clip_coef(g, max_norm, gscale)
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps))
    return p, m, v, g


def adam_torch(p0, grads, lr, dtype, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, gscale=1.0):
    """the same steps by torch on the CPU in `dtype` -> per step (p, m, v) as float64 arrays"""
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(p0)).to(dtype).clone())
    opt = torch.optim.Adam([p], lr=lr, betas=(beta1, beta2), eps=eps, foreach=False)
    out = []
    for g in grads:
        p.grad = torch.from_numpy(np.asarray(g)).to(dtype) * gscale
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        st = opt.state[p]
        out.append(tuple(t.detach().double().numpy().copy() for t in (p, st["exp_avg"], st["exp_avg_sq"])))
    return out


ADAM_N = 4096 * 2 + 333            # two full chunks of the chunked kernel and a partial one whose last workgroup pass is partial
ADAM_LR, ADAM_BETAS, ADAM_EPS = 1e-3, (0.9, 0.999), 1e-8
ADAM_STEPS = 3
# (name, max_norm as a multiple of the first step's gradient norm | 0 = no clipping and no norm at all, gscale)
ADAM_CASES = [("noclip_gs1", 2.0, 1.0), ("clip_gs1", 0.5, 1.0), ("clip_gs_half", 0.5, 0.5), ("clip_gs_third", 0.5, 1.0 / 3.0),
              ("nonorm_gs_third", 0.0, 1.0 / 3.0)]


def adam_inputs():
    """-> (p0 fp32 [n], [g_1, g_2, g_3] fp32): |p0| <= 2^-10; |g| log-uniform over 1e-9 .. 1e+1 with a fixed sign per element (so that m
    does not cancel between the steps: the update stays far above p's rounding) and exact zeros at every 97th element; steps 2 and 3
    rescale the same gradient (x 0.7, x 1.3).  sqrt(v) / sqrt(bc2) runs from ~1e-10 to ~1e+1 across eps = 1e-8."""
    rng = np.random.default_rng(20261018)
    p0 = rng.uniform(-2.0 ** -10, 2.0 ** -10, ADAM_N).astype(np.float32)
    g = (10.0 ** rng.uniform(-9, 1, ADAM_N) * rng.choice([-1.0, 1.0], ADAM_N)).astype(np.float32)
    g[::97] = 0.0
    return p0, [g, (g * np.float32(0.7)).astype(np.float32), (g * np.float32(1.3)).astype(np.float32)]


def adam_case(name):
    """-> dict(max_norm, gscale) of a case of ADAM_CASES; max_norm is a multiple of the norm of the SCALED first gradient, so the
    "noclip" case stays below it in all three steps (1.3 < 2) and the "clip" cases above it (0.7 > 0.5)"""
    _, rel, gscale = next(c for c in ADAM_CASES if c[0] == name)
    _, grads = adam_inputs()
    norm1 = math.sqrt(math.fsum((grads[0].astype(np.float64) * gscale) ** 2))
    return {"max_norm": float(np.float32(rel * norm1)), "gscale": gscale}


def adam_reference_run(name):
    """the float64 run of a case -> list per step of dict(p_old, p, m_old, m, v, g_eff)"""
    c = adam_case(name)
    p0, grads = adam_inputs()
    p, m, v = p0.astype(np.float64), np.zeros(ADAM_N), np.zeros(ADAM_N)
    out = []
    for t, g in enumerate(grads, 1):
        pn, mn, vn, ge = adam_reference(p, g, m, v, t, ADAM_LR, *ADAM_BETAS, ADAM_EPS, c["max_norm"], c["gscale"])
        out.append({"p_old": p, "p": pn, "m_old": m, "m": mn, "v": vn, "g_eff": ge})
        p, m, v = pn, mn, vn
    return out


def half_ulp32(x):
    """half a unit in the last place of the fp32 numbers of magnitude |x| (elementwise)"""
    x = np.abs(np.asarray(x, np.float32))
    return 0.5 * (np.nextafter(x, np.float32(np.inf)).astype(np.float64) - x.astype(np.float64))


def adam_ratios(step_ref, p_old, p_new, m_new, v_new):
    """The three gated quantities of one Adam step as (ours, exact, atol, floor) tuples for conftest.f64_gate / close_ratio.
    p_old, p_new, m_new, v_new: the implementation under test (fp32 values); step_ref: the float64 run's dict of the same step.
      m   : relative to max(|m_old|, |g|) (the lerp m + (g - m)(1 - b1) can cancel), i.e. 1 + (m - m_ref) / scale against 1;
      v   : element-wise relative (a sum of non-negative terms), elements with an exactly zero gradient history left out;
      dp  : p_new - p_old against the float64 update, element-wise relative, with half an ulp of p as the absolute floor
            (the one rounding of p_new that no fp32 implementation can avoid).
    Elements whose gradient is exactly zero must be exactly zero in m, v and dp: asserted here."""
    nz = step_ref["v"] != 0
    m_new, v_new = np.asarray(m_new, np.float64), np.asarray(v_new, np.float64)
    dp = np.asarray(p_new, np.float64) - np.asarray(p_old, np.float64)
    assert not m_new[~nz].any() and not v_new[~nz].any() and not dp[~nz].any(), "a zero gradient must leave m, v and p untouched"
    scale = np.maximum(np.abs(step_ref["m_old"]), np.abs(step_ref["g_eff"]))[nz]
    atol = half_ulp32(np.maximum(np.abs(p_old), np.abs(p_new)))[nz]
    return {"m": (1.0 + (m_new[nz] - step_ref["m"][nz]) / scale, np.ones(int(nz.sum())), 0.0, 0.0),
            "v": (v_new[nz], step_ref["v"][nz], 0.0, 0.0),
            "dp": (dp[nz], (step_ref["p"] - step_ref["p_old"])[nz], atol, 0.0)}


# ---------------------------------------------------------------------------------------------------------------- likelihoods
EB_SHAPES = [(3, 1), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (1, 3), (1, 1)]
EB_NAMES = [f"_{k}{i}" for i in range(5) for k in (("matrix", "bias", "factor") if i < 4 else ("matrix", "bias"))]


def eb_random_pack(C, seed):
    """[C,58] EntropyBottleneck parameters in the layout of orc.eb_pack_params (per layer: matrix, bias, factor): CompressAI's
    initialisation (filters 3-3-3-3: matrix = log(expm1(1 / scale / fan_out)), bias in (-1/2, 1/2)) at init_scale 1 -- a density
    about one quantisation bin wide, whose tails reach the 1e-9 floor near |z| = 20 -- with every value perturbed and non-zero gate
    factors, so that no term of the MLP drops out."""
    rng = np.random.default_rng(seed)
    filters = (1, 3, 3, 3, 3, 1)
    scale = 1.0
    cols = []
    for i in range(5):
        init = math.log(math.expm1(1.0 / scale / filters[i + 1]))
        cols.append(init + rng.uniform(-0.3, 0.3, (C, filters[i + 1] * filters[i])))
        cols.append(rng.uniform(-0.5, 0.5, (C, filters[i + 1])))
        if i < 4:
            cols.append(rng.uniform(-0.4, 0.4, (C, filters[i + 1])))
    pack = np.concatenate(cols, axis=1).astype(np.float32)
    assert pack.shape == (C, 58)
    return pack


def eb_state_dict(pack, dtype):
    """the 14 tensors of an EntropyBottleneck from its [C,58] pack (the inverse of orc.eb_pack_params)"""
    sd, o = {}, 0
    for n, s in zip(EB_NAMES, EB_SHAPES):
        k = s[0] * s[1]
        sd["entropy_bottleneck." + n] = torch.from_numpy(np.ascontiguousarray(pack[:, o:o + k])).to(dtype).reshape(-1, *s)
        o += k
    return sd


def eb_likelihood(z_hat, pack, dtype=torch.float64):
    """z_hat [npix, C] (the noisy latent) -> likelihoods [npix, C] as float64, computed in `dtype`"""
    import stem_torch_cpu as stc
    v = torch.from_numpy(np.ascontiguousarray(np.asarray(z_hat).T)).to(dtype).unsqueeze(1)          # [C, 1, npix]
    with torch.no_grad():
        lik = stc.eb_likelihood(eb_state_dict(np.asarray(pack), dtype), v)
    return lik.squeeze(1).T.double().numpy()


def gc_likelihood(out, scales, means, dtype=torch.float64):
    import stem_torch_cpu as stc
    o, s, m = (torch.from_numpy(np.ascontiguousarray(a)).to(dtype) for a in (out, scales, means))
    with torch.no_grad():
        return stc.gc_likelihood(o, s, m).double().numpy()


def gc_backward(out, scales, means, coef, dtype=torch.float64):
    """-> (dscales, dmeans) of coef * sum(ln likelihood) by autograd (d / d likelihood = coef / likelihood), float64 arrays"""
    import stem_torch_cpu as stc
    o, s, m = (torch.from_numpy(np.ascontiguousarray(a)).to(dtype) for a in (out, scales, means))
    s.requires_grad_(True)
    m.requires_grad_(True)
    (coef * torch.log(stc.gc_likelihood(o, s, m)).sum()).backward()
    return s.grad.double().numpy(), m.grad.double().numpy()


# (B, H, W, C): C = 3 and 5 so that the noise lane i & 3 does not line up with the channel; 4096 pixels is the last size of the
# per-channel EntropyBottleneck kernel, 4160 the per-element one
TAIL_SHAPES = [(2, 9, 11, 3), (1, 64, 64, 5), (1, 64, 65, 3), (1, 64, 65, 5)]


def gc_inputs(B, H, W, C, seed, tie=False):
    """-> (y, noise, scales, means) as [npix, C] fp32.  scales log-uniform over 0.01 .. 10 (a quarter below scale_bound = 0.11), every
    16th element 7 or more away from its mean at a scale <= 1 (likelihood below the 1e-9 floor); tie: every 13th element has
    y + noise == mean exactly."""
    rng = np.random.default_rng(seed)
    n = B * H * W
    scales = (10.0 ** rng.uniform(-2, 1, (n, C))).astype(np.float32)
    means = rng.uniform(-3, 3, (n, C)).astype(np.float32)
    y = (means + rng.standard_normal((n, C)) * np.maximum(scales, 0.11) * 1.5).astype(np.float32)
    noise = rng.uniform(-0.5, 0.5, (n, C)).astype(np.float32)
    far = np.zeros(n * C, bool)
    far[5::16] = True
    far = far.reshape(n, C)
    scales[far] = np.minimum(scales[far], 1.0)
    y[far] = (means[far] + rng.choice([-1.0, 1.0], int(far.sum())) * rng.uniform(7.0, 9.0, int(far.sum()))).astype(np.float32)
    if tie:
        t = np.zeros(n * C, bool)
        t[3::13] = True
        t = t.reshape(n, C)
        y[t], noise[t] = means[t], 0.0
    return y, noise, scales, means


def eb_inputs(B, H, W, C, seed):
    """-> (z, noise) as [npix, C] fp32: z normal with sigma 3, every 16th element 22 .. 30 away from 0 (likelihood at the floor)"""
    rng = np.random.default_rng(seed)
    n = B * H * W
    z = (rng.standard_normal((n, C)) * 3.0).astype(np.float32)
    far = np.zeros(n * C, bool)
    far[7::16] = True
    far = far.reshape(n, C)
    z[far] = (rng.choice([-1.0, 1.0], int(far.sum())) * rng.uniform(22.0, 30.0, int(far.sum()))).astype(np.float32)
    return z, rng.uniform(-0.5, 0.5, (n, C)).astype(np.float32)
