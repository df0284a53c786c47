"""Float64 references for the EntropyBottleneck kernels of any `filters` tuple (csrc/eb_filters.hip, include/stem_eb_filters.h).

No GPU and nothing of the package's native code: a torch-CPU statement of `_logits_cumulative` (compressai/entropy_models/
entropy_models.py:388-407), the likelihood with the LowerBound gradient rule (ops/bound_ops.py:28-31), the per-sample backward and
the auxiliary loss, for widths = (1, *filters, 1).  Run in float64 it is the reference, run in float32 the yardstick.
tests/test_eb_filters_ref.py pins it against the reference's own module (tests/golden/eb_filters.npz) and against entropy_ref at
(3, 3, 3, 3); tests/test_hip_eb_filters.py compares the HIP kernels with it.

Built like entropy_ref.eb_backward / eb_aux: every sample gets parameters of its own (the channel's row repeated), so the gradient
of one scalar with respect to the repeated parameters is the per-sample gradient.  The input makers are train_tail_ref.eb_random_pack
/ eb_inputs for any widths: initial values at init_scale 1 plus uniform(+-0.3) on the matrices, uniform(+-0.5) biases,
uniform(+-0.4) factors.
"""
import functools
import math

import numpy as np
import torch

import train_tail_ref as ref

LIK_BOUND = 1e-9
TUPLES = ((), (1,), (5,), (3, 3, 3), (3, 3, 3, 3), (2, 4, 8), (8,) * 6)
GOLDEN_TUPLES = ((), (1,), (5,), (3, 3, 3), (2, 4, 8), (8,) * 6)
REGIMES = ("train", "mixed")
MAX_FILTERS, MAX_WIDTH, MAX_NPARAM = 6, 8, 433
AUX_TARGET = np.array([-math.log(2.0 / 1e-9 - 1.0), 0.0, math.log(2.0 / 1e-9 - 1.0)], np.float32)


def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def tuple_id(filters):
    return "f" + ("-".join(str(f) for f in filters) if filters else "none")


# ---------------------------------------------------------------------------------------------------------------- layout
def layout(filters):
    """-> [(name, shape per channel, offset, length)] of the 3 L + 2 tensors in pack order: per layer matrix (out x in, row major),
    bias, factor (every layer but the last).  The numpy statement F.ebf_layout is compared with."""
    widths = (1, *filters, 1)
    out, off = [], 0
    for i in range(len(filters) + 1):
        fan_in, fan_out = widths[i], widths[i + 1]
        groups = [(f"_matrix{i}", (fan_out, fan_in)), (f"_bias{i}", (fan_out, 1))]
        if i < len(filters):
            groups.append((f"_factor{i}", (fan_out, 1)))
        for name, shape in groups:
            out.append((name, shape, off, shape[0] * shape[1]))
            off += shape[0] * shape[1]
    return out


def nparam(filters):
    return sum(n for _, _, _, n in layout(filters))


def random_pack(C, filters, seed):
    """[C, nparam] parameters: train_tail_ref.eb_random_pack for any widths (the same draws, in the same order, at (3, 3, 3, 3))"""
    rng = np.random.default_rng(seed)
    widths = (1, *filters, 1)
    cols = []
    for i in range(len(filters) + 1):
        init = math.log(math.expm1(1.0 / 1.0 / widths[i + 1]))
        cols.append(init + rng.uniform(-0.3, 0.3, (C, widths[i + 1] * widths[i])))
        cols.append(rng.uniform(-0.5, 0.5, (C, widths[i + 1])))
        if i < len(filters):
            cols.append(rng.uniform(-0.4, 0.4, (C, widths[i + 1])))
    pack = np.concatenate(cols, axis=1).astype(np.float32)
    assert pack.shape == (C, nparam(filters))
    return pack


def tensors_of(pack, filters, dtype=torch.float64):
    """{name: [rows, out, in] tensor} of a [rows, nparam] pack"""
    pack = np.asarray(pack)
    return {name: torch.from_numpy(np.ascontiguousarray(pack[:, o:o + n])).to(dtype).reshape(-1, *shape)
            for name, shape, o, n in layout(filters)}


def pack_columns(dpack, filters):
    """[C, nparam] -> the (name, [C, len]) column groups of the parameter tensors"""
    return [(name, np.asarray(dpack)[:, o:o + n]) for name, _, o, n in layout(filters)]


# ---------------------------------------------------------------------------------------------------------------- the density
def logits_cumulative(t, filters, v):
    """entropy_models.py:388-407: v [rows, 1, M] -> [rows, 1, M]"""
    x = v
    for i in range(len(filters) + 1):
        x = torch.matmul(torch.nn.functional.softplus(t[f"_matrix{i}"]), x) + t[f"_bias{i}"]
        if i < len(filters):
            x = x + torch.tanh(t[f"_factor{i}"]) * torch.tanh(x)
    return x


class _LowerBound(torch.autograd.Function):
    """max(x, bound) whose gradient passes where x >= bound or the gradient is negative (ops/bound_ops.py:28-31)"""

    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x)
        ctx.bound = bound
        return torch.clamp(x, min=bound)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * ((x >= ctx.bound) | (g < 0)).to(g.dtype), None


def _raw(t, filters, v):
    lower, upper = logits_cumulative(t, filters, v - 0.5), logits_cumulative(t, filters, v + 0.5)
    sign = -torch.sign(lower + upper).detach()
    return torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower))


def raw_likelihood(z_hat, pack, filters, dtype=torch.float64):
    """z_hat [npix, C] -> |sigmoid(s upper) - sigmoid(s lower)| before the floor, [npix, C] float64, computed in `dtype`"""
    v = torch.from_numpy(np.ascontiguousarray(np.asarray(z_hat, np.float32).T)).to(dtype).unsqueeze(1)      # [C, 1, npix]
    with torch.no_grad():
        raw = _raw(tensors_of(np.asarray(pack, np.float32), filters, dtype), filters, v)
    return raw.squeeze(1).T.double().numpy()


def likelihood(z_hat, pack, filters, dtype=torch.float64, bound=LIK_BOUND):
    return np.maximum(raw_likelihood(z_hat, pack, filters, dtype), bound)


def backward(z_hat, pack, dlik, filters, dtype=torch.float64, bound=LIK_BOUND):
    """z_hat, dlik [npix, C], pack [C, nparam] -> (dz [npix, C], dpack [C, nparam]) as float64 arrays, computed in `dtype`: sample
    pix * C + c has row c of the pack as parameters of its own; the per-sample gradients are summed over pixels afterwards"""
    z_hat, dlik = np.asarray(z_hat, np.float32), np.asarray(dlik, np.float32)
    npix, C = z_hat.shape
    N, NP = npix * C, nparam(filters)
    t = tensors_of(np.tile(np.asarray(pack, np.float32), (npix, 1)), filters, dtype)       # row pix * C + c = pack[c]
    t = {k: x.clone().requires_grad_(True) for k, x in t.items()}
    params = [t[name] for name, _, _, _ in layout(filters)]
    v = torch.from_numpy(z_hat.reshape(-1).copy()).to(dtype).reshape(N, 1, 1).requires_grad_(True)
    g = torch.from_numpy(dlik.reshape(-1).copy()).to(dtype).reshape(N, 1, 1)
    lik = _LowerBound.apply(_raw(t, filters, v), bound)
    grads = torch.autograd.grad((lik * g).sum(), [v] + params)
    dz = grads[0].reshape(npix, C).double().numpy()
    dpack = torch.cat([x.reshape(N, -1) for x in grads[1:]], dim=1).reshape(npix, C, NP).sum(0).double().numpy()
    return dz, dpack


def aux(quantiles, pack, target, filters, dtype=torch.float64):
    """EntropyBottleneck.loss (entropy_models.py:383-386) -> (loss, dq [C, 1, 3]) in float64, computed in `dtype`"""
    t = tensors_of(np.asarray(pack, np.float32), filters, dtype)
    q = torch.from_numpy(np.asarray(quantiles, np.float32).copy()).to(dtype).requires_grad_(True)
    tg = torch.from_numpy(np.asarray(target, np.float32).copy()).to(dtype).reshape(1, 1, 3)
    loss = torch.abs(logits_cumulative(t, filters, q) - tg).sum()
    loss.backward()
    return float(loss.detach().double()), q.grad.double().numpy()


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def forward_case(shape, filters):
    """-> dict(z, noise, z_hat [npix, C], pack, medians [C]) fp32, read-only: train_tail_ref.eb_inputs(seed 31), the pack of seed 32"""
    B, H, W, C = shape
    z, noise = ref.eb_inputs(B, H, W, C, 31)
    medians = np.random.default_rng(33).uniform(-1.0, 1.0, C).astype(np.float32)
    return _frozen(z=z, noise=noise, z_hat=z + noise, pack=random_pack(C, filters, 32), medians=medians)


@functools.lru_cache(maxsize=None)
def backward_case(shape, filters, regime):
    """-> dict(z_hat, pack, dlik, raw, blocked), entropy_ref.eb_backward_case for any filters:
      train: dlik = fl32(coef) / fl32(max(raw, 1e-9)), coef = -1 / (ln 2 npix): negative everywhere, nothing is blocked
      mixed: |dlik| uniform in [0.5, 2] with a random sign: blocked where raw < 1e-9 and dlik > 0"""
    B, H, W, C = shape
    c = forward_case(shape, filters)
    raw = raw_likelihood(c["z_hat"], c["pack"], filters)
    if regime == "train":
        coef = np.float32(-1.0 / (math.log(2.0) * B * H * W))
        dlik = (coef / np.maximum(raw, LIK_BOUND).astype(np.float32)).astype(np.float32)
    else:
        rng = np.random.default_rng(5)
        dlik = (rng.uniform(0.5, 2.0, raw.shape) * rng.choice([-1.0, 1.0], raw.shape)).astype(np.float32)
    blocked = (raw < LIK_BOUND) & ~(dlik < 0)
    return _frozen(z_hat=c["z_hat"], pack=c["pack"], dlik=dlik, raw=raw, blocked=blocked)


@functools.lru_cache(maxsize=None)
def backward_reference(shape, filters, regime):
    """-> dict(dz, dpack: the float64 run; dz32, dpack32: the float32 run of the same code, the yardstick), computed once"""
    c = backward_case(shape, filters, regime)
    dz, dpack = backward(c["z_hat"], c["pack"], c["dlik"], filters)
    dz32, dpack32 = backward(c["z_hat"], c["pack"], c["dlik"], filters, torch.float32)
    return _frozen(dz=dz, dpack=dpack, dz32=dz32, dpack32=dpack32)


@functools.lru_cache(maxsize=None)
def aux_inputs(C, filters, seed=70):
    """-> (quantiles [C, 1, 3] uniform in (-8, 8), pack [C, nparam], target [3]) fp32, read-only"""
    pack = random_pack(C, filters, seed + C)
    q = np.random.default_rng(seed + 1000 + C).uniform(-8.0, 8.0, (C, 1, 3)).astype(np.float32)
    return tuple(_frozen(q=q, pack=pack, target=AUX_TARGET.copy()).values())


@functools.lru_cache(maxsize=None)
def aux_reference(C, filters):
    q, pack, target = aux_inputs(C, filters)
    loss, dq = aux(q, pack, target, filters)
    loss32, dq32 = aux(q, pack, target, filters, torch.float32)
    return _frozen(loss=loss, dq=dq, loss32=loss32, dq32=dq32)


# ---------------------------------------------------------------------------------------------------------------- the gate
def gate_rtol(ref32_ratio):
    """The bound of conftest.f64_gate for a tensor whose float32 reference run is `ref32_ratio` (conftest.close_ratio, floor 0.1) from
    the float64 one: 1e-4, and max(1e-4, 3 x that distance) where the reference itself is more than 3.3e-5 away
    (tests/test_hip_spread.py's rule).  -> (rtol, widened)"""
    widened = ref32_ratio > 3.3e-5
    return (max(1e-4, 3.0 * ref32_ratio) if widened else 1e-4), widened
