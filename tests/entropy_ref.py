"""Float64 references for the entropy-model kernels next to the fused training forward: the EntropyBottleneck backward, its auxiliary
loss, the eval-mode / explicit-noise forwards, the stand-alone GaussianConditional backward and the table indexes.

No GPU and nothing of the package's native code: tests/test_entropy_ref.py pins these functions and the preconditions of their inputs
on the CPU, tests/test_hip_entropy_ops.py compares the HIP kernels of csrc/entropy.hip with them.  The likelihood functions, packs
and input generators are those of tests/train_tail_ref.py.

  eb_backward            d (lik . dlik).sum() / d (z_hat, pack) by autograd through oracle/stem_torch_cpu.py (_eb_logits, lower_bound
                         with its LowerBound gradient rule), every sample with parameters of its own, so that one autograd call gives
                         the per-sample parameter gradients: their sum over pixels is dpack, the sum of their magnitudes per branch is
                         A, the quantity an fp32 summation error is relative to
  eb_backward_case       the inputs of the two gradient regimes (train: dlik = coef / lik; mixed: random signs, blocked elements)
  eb_aux / aux_inputs    EntropyBottleneck.loss (stc.eb_aux_loss) and d loss / d quantiles
  eb_eval_inputs /       latents with exact rounding ties (median + k + 1/2, k even and odd) for the eval-mode forwards
  gc_eval_inputs
  index_scales /         scales at, just below and just above every entry of a scale table, and the plain statement of
  build_indexes          GaussianConditional.build_indexes
"""
import functools
import math

import numpy as np
import torch

import train_tail_ref as ref
from train_tail_ref import EB_NAMES, EB_SHAPES, TAIL_SHAPES, eb_random_pack, eb_state_dict  # noqa: F401

LIK_BOUND, SCALE_BOUND = 1e-9, 0.11
EB_LEN = [a * b for a, b in EB_SHAPES]                             # == kLen of csrc/entropy.hip
EB_OFF = [int(o) for o in np.cumsum([0] + EB_LEN[:-1])]            # == kOff, the columns of orc.eb_unpack_grads
NP = sum(EB_LEN)
assert NP == 58


def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------------------------------------------- EntropyBottleneck backward
def eb_raw_likelihood(z_hat, pack, dtype=torch.float64):
    """|sigmoid(sign upper) - sigmoid(sign lower)| BEFORE the 1e-9 floor, [npix, C] float64 (what the LowerBound rule looks at)"""
    import stem_torch_cpu as stc
    v = torch.from_numpy(np.ascontiguousarray(np.asarray(z_hat, np.float32).T)).to(dtype).unsqueeze(1)      # [C, 1, npix]
    sd = eb_state_dict(np.array(pack, np.float32), dtype)
    with torch.no_grad():
        lower, upper = stc._eb_logits(sd, v - 0.5), stc._eb_logits(sd, v + 0.5)
        sign = -torch.sign(lower + upper)
        raw = torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower))
    return raw.squeeze(1).T.double().numpy()


def eb_backward(z_hat, pack, dlik, dtype=torch.float64, with_A=True):
    """z_hat, dlik [npix, C], pack [C, 58] -> (dz [npix, C], dpack [C, 58], A [C, 58] or None) as float64 arrays, computed in `dtype`.
    Sample pix * C + c gets row c of the pack as parameters of its own, so the gradient of the one scalar (lik * dlik).sum() with
    respect to the repeated parameters is the per-sample gradient.  A[c, k] = sum over pixels of |upper-branch term| +
    |lower-branch term| of parameter k: sigmoid(sign upper) and sigmoid(sign lower) differentiated separately, with the pass mask of
    the LowerBound rule and the sign of the difference applied as constants."""
    import stem_torch_cpu as stc
    z_hat, dlik = np.asarray(z_hat, np.float32), np.asarray(dlik, np.float32)
    npix, C = z_hat.shape
    N = npix * C
    sd = eb_state_dict(np.tile(np.asarray(pack, np.float32), (npix, 1)), dtype)          # row pix * C + c = pack[c]
    sd = {k: t.clone().requires_grad_(True) for k, t in sd.items()}
    params = [sd["entropy_bottleneck." + n] for n in EB_NAMES]
    v = torch.from_numpy(z_hat.reshape(-1).copy()).to(dtype).reshape(N, 1, 1).requires_grad_(True)
    g = torch.from_numpy(dlik.reshape(-1).copy()).to(dtype).reshape(N, 1, 1)
    lower, upper = stc._eb_logits(sd, v - 0.5), stc._eb_logits(sd, v + 0.5)
    sign = -torch.sign(lower + upper).detach()
    su, sl = torch.sigmoid(sign * upper), torch.sigmoid(sign * lower)
    raw = torch.abs(su - sl)
    lik = stc.lower_bound(raw, LIK_BOUND)
    grads = torch.autograd.grad((lik * g).sum(), [v] + params, retain_graph=with_A)

    def rows(gs):
        return torch.cat([t.reshape(N, -1) for t in gs], dim=1)                           # [N, 58] in pack order

    dz = grads[0].reshape(npix, C).double().numpy()
    dpack = rows(grads[1:]).reshape(npix, C, NP).sum(0).double().numpy()
    if not with_A:
        return dz, dpack, None
    gd = (g * ((raw >= LIK_BOUND) | (g < 0)).to(dtype) * torch.sign(su - sl)).detach()
    gu = rows(torch.autograd.grad((su * gd).sum(), params, retain_graph=True))
    gl = rows(torch.autograd.grad((-sl * gd).sum(), params))
    A = (gu.abs() + gl.abs()).reshape(npix, C, NP).sum(0).double().numpy()
    return dz, dpack, A


EB_REGIMES = ("train", "mixed")


@functools.lru_cache(maxsize=None)
def eb_backward_case(shape, regime):
    """-> dict(z_hat, pack, dlik, raw, blocked) of read-only arrays: z_hat = z + noise of eb_inputs(seed 31), the pack of seed 32 (the
    inputs of test_eb_forward_train_vs_float64); raw: the float64 likelihood before the floor.
      train: dlik = fl32(coef) / fl32(max(raw, 1e-9)), coef = -1 / (ln 2 npix): negative everywhere, nothing is blocked
      mixed: |dlik| uniform in [0.5, 2] with a random sign: blocked where raw < 1e-9 and dlik > 0"""
    B, H, W, C = shape
    z, noise = ref.eb_inputs(B, H, W, C, 31)
    pack = eb_random_pack(C, 32)
    z_hat = z + noise
    raw = eb_raw_likelihood(z_hat, pack)
    if regime == "train":
        coef = np.float32(-1.0 / (math.log(2.0) * B * H * W))
        dlik = (coef / np.maximum(raw, LIK_BOUND).astype(np.float32)).astype(np.float32)
    else:
        rng = np.random.default_rng(5)
        dlik = (rng.uniform(0.5, 2.0, z.shape) * rng.choice([-1.0, 1.0], z.shape)).astype(np.float32)
    blocked = (raw < LIK_BOUND) & ~(dlik < 0)
    return _frozen(z_hat=z_hat, pack=pack, dlik=dlik, raw=raw, blocked=blocked)


@functools.lru_cache(maxsize=None)
def eb_backward_reference(shape, regime):
    """-> dict(dz, dpack, A: the float64 run; dz32, dpack32: the float32 run of the same code, the yardstick) of a case, computed once"""
    c = eb_backward_case(shape, regime)
    dz, dpack, A = eb_backward(c["z_hat"], c["pack"], c["dlik"])
    dz32, dpack32, _ = eb_backward(c["z_hat"], c["pack"], c["dlik"], torch.float32, with_A=False)
    return _frozen(dz=dz, dpack=dpack, A=A, dz32=dz32, dpack32=dpack32)


def pack_columns(dpack):
    """[C, 58] -> the 14 (name, [C, len]) column groups of the parameter tensors"""
    return [(n, np.asarray(dpack)[:, o:o + k]) for n, o, k in zip(EB_NAMES, EB_OFF, EB_LEN)]


# ---------------------------------------------------------------------------------------------------------------- auxiliary loss
# 1; 85 | 86: 255 | 258 items, the 256-thread kernel's second workgroup and its atomic; 256: 768 items, exactly one pass of the block
# kernel (the training model); 257: a second pass of three items; 320; 688: the most the block kernel's LDS holds
AUX_CHANNELS = (1, 85, 86, 256, 257, 320, 688)
AUX_MAX_C = 688
AUX_TARGET = np.array([-math.log(2.0 / 1e-9 - 1.0), 0.0, math.log(2.0 / 1e-9 - 1.0)], np.float32)


@functools.lru_cache(maxsize=None)
def aux_inputs(C, seed=70):
    """-> (quantiles [C,1,3] uniform in (-8, 8), pack [C,58], target [3]) fp32, read-only"""
    pack = eb_random_pack(C, seed + C)
    q = np.random.default_rng(seed + 1000 + C).uniform(-8.0, 8.0, (C, 1, 3)).astype(np.float32)
    return tuple(_frozen(q=q, pack=pack, target=AUX_TARGET.copy()).values())


def eb_aux(quantiles, pack, target, dtype=torch.float64):
    """-> (loss, dq [C,1,3], d [C,1,3] = logits(quantiles) - target) in float64, computed in `dtype`"""
    import stem_torch_cpu as stc
    sd = eb_state_dict(np.array(pack, np.float32), dtype)
    q = torch.from_numpy(np.asarray(quantiles, np.float32).copy()).to(dtype).requires_grad_(True)
    sd["entropy_bottleneck.quantiles"] = q
    t = torch.from_numpy(np.asarray(target, np.float32).copy()).to(dtype).reshape(1, 1, 3)
    loss = stc.eb_aux_loss(sd, t)
    loss.backward()
    with torch.no_grad():
        d = stc._eb_logits(sd, q, stop_gradient=True) - t
    return float(loss.detach().double()), q.grad.double().numpy(), d.double().numpy()


@functools.lru_cache(maxsize=None)
def aux_reference(C):
    q, pack, target = aux_inputs(C)
    loss, dq, d = eb_aux(q, pack, target)
    loss32, dq32, _ = eb_aux(q, pack, target, torch.float32)
    return _frozen(loss=loss, dq=dq, d=d, loss32=loss32, dq32=dq32)


# ---------------------------------------------------------------------------------------------------------------- eval-mode inputs
EB_TIE_K = (-3, 2, 0, -1)            # odd, even, even, odd: pixel j of every channel is median + k_j + 1/2


def eb_eval_inputs(B, H, W, C, seed):
    """-> (z [npix, C], medians [C]) fp32: eb_inputs with medians that are multiples of 1/64 in [-2, 2] and, in every channel, the
    first four pixels at median + k + 1/2 (k = -3, 2, 0, -1), exactly representable, so that z - median is an exact rounding tie"""
    z, _ = ref.eb_inputs(B, H, W, C, seed)
    med = (np.random.default_rng(seed + 1).integers(-128, 129, C) / 64.0).astype(np.float32)
    for j, k in enumerate(EB_TIE_K):
        z[j] = med + np.float32(k + 0.5)
    return z, med


GC_TIE_K = (-2, -1, 0, 1, 3)


def gc_tie_mask(n, C):
    t = np.zeros(n * C, bool)
    t[3::13] = True
    return t.reshape(n, C)


def gc_eval_inputs(B, H, W, C, seed):
    """-> (y, scales, means) fp32 [npix, C]: gc_inputs, with every 13th element a rounding tie: its mean a multiple of 1/64 and
    y = mean + k + 1/2 exactly, k cycling through -2, -1, 0, 1, 3"""
    y, _, scales, means = ref.gc_inputs(B, H, W, C, seed)
    t = gc_tie_mask(B * H * W, C)
    means[t] = (np.round(means[t] * 64.0) / 64.0).astype(np.float32)
    k = np.resize(np.array(GC_TIE_K, np.float32), int(t.sum()))
    y[t] = means[t] + (k + np.float32(0.5))
    return y, scales, means


def round_about(x, m):
    """rint(x - m) + m in fp32 (numpy rounds half to even), m broadcast"""
    x, m = np.asarray(x, np.float32), np.asarray(m, np.float32)
    return (np.rint(x - m).astype(np.float32) + m).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- table indexes
INDEX_SHAPE = (1, 19, 9, 3)          # 513 scales: two full 256-thread workgroups and one element


def index_scales(table):
    """-> [npix, C] fp32 scales of INDEX_SHAPE: every table entry t, nextafter(t, +inf), nextafter(t, -inf); 0, 0.11 and its
    neighbours, a value above the last entry; the rest log-uniform over 0.01 .. 2 x the last entry"""
    table = np.asarray(table, np.float32)
    B, H, W, C = INDEX_SHAPE
    up, down = np.float32(np.inf), np.float32(-np.inf)
    sb = np.float32(SCALE_BOUND)
    special = np.concatenate([table, np.nextafter(table, up), np.nextafter(table, down),
                              np.array([0.0, sb, np.nextafter(sb, up), np.nextafter(sb, down), table[-1] * np.float32(1.5)], np.float32)])
    n = B * H * W * C
    assert special.size < n and n % 256 != 0
    rng = np.random.default_rng(91)
    fill = (10.0 ** rng.uniform(-2.0, math.log10(2.0 * float(table[-1])), n - special.size)).astype(np.float32)
    s = np.concatenate([special, fill]).astype(np.float32)
    return s[rng.permutation(n)].reshape(B * H * W, C)


def build_indexes(scales, table):
    """min(searchsorted(table[:-1], max(s, 0.11), 'left'), T - 1): the number of the first T - 1 entries below the bounded scale"""
    table = np.asarray(table, np.float32)
    s = np.maximum(np.asarray(scales, np.float32), np.float32(SCALE_BOUND))
    return np.minimum(np.searchsorted(table[:-1], s, side="left"), len(table) - 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- log2 sum
LOG2_SIZES = (1, 256 * 1024, 256 * 1024 + 1, 3 * 256 * 1024 + 77)          # one element; the full grid once; one element of a second
#                                                                            trip of the grid-stride loop; three trips and a partial one


@functools.lru_cache(maxsize=None)
def log2_likelihoods():
    """the largest of LOG2_SIZES log-uniform likelihoods in [1e-9, 1], with both ends present among the first elements"""
    lik = (10.0 ** np.random.default_rng(95).uniform(-9.0, 0.0, LOG2_SIZES[-1])).astype(np.float32)
    lik[0] = 1e-9
    lik = np.clip(lik, np.float32(1e-9), np.float32(1.0))
    lik.setflags(write=False)
    return lik
