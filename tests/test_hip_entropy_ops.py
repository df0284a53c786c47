"""GPU parity tests, op level, for the entropy-model kernels of csrc/entropy.hip that run next to the fused training forward: the
EntropyBottleneck backward (256 threads per channel, 58 parameter gradients per thread, shuffle + LDS reduction), its auxiliary loss
(both kernels), the eval-mode and explicit-noise forwards, the stand-alone GaussianConditional backward, the table indexes, the log2
sum and the parameter pack / unpack.

Each kernel is called on its own and compared with a plain reference of the same operation (tests/entropy_ref.py, pinned on the CPU
by tests/test_entropy_ref.py, which also shows the preconditions of the inputs): bit for bit where the operation is exact (rounding
to integers, one fp32 add, copies, maxima, integer indexes), through conftest.f64_gate at the project's 1e-4 against float64 where it
is fp32 arithmetic.  Shapes: train_tail_ref.TAIL_SHAPES -- 198 pixels (less than one pass of a 256-thread workgroup), 4096 (16 passes;
the last size of the per-channel forward kernel), 4160 (16 passes and a partial one; the per-element forward kernel), C = 3 and 5."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import entropy_ref as er
import train_tail_ref as ref
from conftest import REPO, assert_close, close_ratio, f64_gate
from test_hip_train_tail import flat, nhwc, rec_max, vec

sys.path.insert(0, os.path.join(REPO, "oracle"))
import stem_oracle as orc  # noqa: E402

# the references hand out read-only arrays (shared between tests); torch warns when it wraps one without copying
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return functional


def _id(s):
    return "B%d_%dx%d_C%d" % s


def rec_slots(q):
    """a scale record (stem_common.h) -> its slots as a numpy array"""
    q = q.cpu()
    ns = int(q[:1].view(torch.int32)[0])
    assert 0 < ns <= q.numel() - 16
    return q[16:16 + ns].numpy()


# =========================================================================================================== 1. eb_backward
@pytest.mark.parametrize("regime", er.EB_REGIMES)
@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_id)
def test_eb_backward_vs_float64(F, shape, regime):
    """stem_eb_backward(_rec) against float64 autograd: dz and the 14 parameter tensors of dpack through f64_gate (1e-4, floor 0.1),
    the float32 run of the reference printed as the yardstick; max |dpack - exact| / A printed (A: the sum of the magnitudes of the
    summed terms; informational).  Exact: blocked elements (LowerBound rule: raw likelihood below 1e-9 and dlik >= 0) are zero, or
    dzhat_in where given; dzhat_in is one fp32 add; the record holds C slots with max |dz[:, c]|; record=True changes no bit; two calls
    agree bit for bit (fixed-order reduction, no atomics).  "train": dlik = coef / lik, all negative; "mixed": random signs."""
    B, H, W, C = shape
    c, r = er.eb_backward_case(shape, regime), er.eb_backward_reference(shape, regime)
    what = f"eb_backward {regime} {_id(shape)}"
    zh, pd, dl = nhwc(c["z_hat"], B, H, W), vec(c["pack"]), nhwc(c["dlik"], B, H, W)
    dz_t, dpack_t = F.eb_backward(zh, pd, dl)
    dz, dpack = flat(dz_t), dpack_t.cpu().numpy()
    f64_gate(dz, r["dz"], close_ratio(r["dz32"], r["dz"], 0.1), what + " dz")
    for (name, got), (_, exact), (_, y32) in zip(er.pack_columns(dpack), er.pack_columns(r["dpack"]), er.pack_columns(r["dpack32"])):
        f64_gate(got, exact, close_ratio(y32, exact, 0.1), f"{what} dpack{name}")
    print(f"[A-relative] {what}: max |dpack - exact| / A = {(np.abs(dpack - r['dpack']) / r['A']).max():.3e}   "
          f"reference-fp32 {(np.abs(r['dpack32'] - r['dpack']) / r['A']).max():.3e}")
    blocked = c["blocked"]
    assert blocked.any() == (regime == "mixed")
    assert np.array_equal(dz[blocked], np.zeros(int(blocked.sum()), np.float32)) and np.array_equal(dz != 0, r["dz"] != 0)
    # dzhat_in: one fp32 add per element
    dzin = np.random.default_rng(6).uniform(-1.0, 1.0, dz.shape).astype(np.float32) * np.float32(np.abs(dz).max())
    dz_w, dpack_w = F.eb_backward(zh, pd, dl, dzhat_in=nhwc(dzin, B, H, W))
    assert np.array_equal(flat(dz_w), dz + dzin) and torch.equal(dpack_w, dpack_t)
    assert np.array_equal(flat(dz_w)[blocked], dzin[blocked])
    # the record: one slot per channel, max |dz[:, c]|; nothing else changes; a second call gives the same bits
    for dzin_t, base in ((None, dz_t), (nhwc(dzin, B, H, W), dz_w)):
        dz_r, dpack_r, q = F.eb_backward(zh, pd, dl, dzhat_in=dzin_t, record=True)
        assert np.array_equal(rec_slots(q), np.abs(flat(base)).max(0)) and rec_slots(q).size == C
        assert torch.equal(dz_r, base) and torch.equal(dpack_r, dpack_t)


def test_eb_backward_channels_do_not_leak(F):
    """row c of dpack from a C-channel call == the row of a one-channel call on channel c alone, bit for bit (c = 0 and C - 1; 4160
    pixels): nothing crosses between workgroups through red[][] / prep[], and the channel stride of the loads is right"""
    shape = ref.TAIL_SHAPES[3]
    B, H, W, C = shape
    c = er.eb_backward_case(shape, "mixed")
    dz_t, dpack_t = F.eb_backward(nhwc(c["z_hat"], B, H, W), vec(c["pack"]), nhwc(c["dlik"], B, H, W))
    for ch in (0, C - 1):
        one = slice(ch, ch + 1)
        dz1, dpack1 = F.eb_backward(nhwc(c["z_hat"][:, one], B, H, W), vec(c["pack"][one]), nhwc(c["dlik"][:, one], B, H, W))
        assert torch.equal(dpack1[0], dpack_t[ch]) and np.array_equal(flat(dz1)[:, 0], flat(dz_t)[:, ch])


# =========================================================================================================== 2. auxiliary loss
@pytest.mark.parametrize("C", er.AUX_CHANNELS)
def test_eb_aux_loss_vs_float64(F, C):
    """stem_eb_aux_loss_grad (one 768-thread workgroup, C x 58 floats of dynamic LDS, 3 C items in passes of 768) and stem_eb_aux_loss
    (256-thread workgroups, one atomic each) against stc.eb_aux_loss in float64: the loss, a sum of 3 C non-negative terms, at 1e-4
    relative; dq element-wise at 1e-4, floor 0.1.  accumulate=True adds in one fp32 add; loss_out is the tensor handed in.  The
    largest difference between the two kernels' dq is printed (no assertion: their bodies may be contracted differently)."""
    q, pack, target = er.aux_inputs(C)
    r = er.aux_reference(C)
    qd, pd, td = vec(q), vec(pack), vec(target)
    dq_t = torch.full((C, 1, 3), float("nan"), device="cuda")
    loss_in = torch.full((1,), float("nan"), device="cuda")
    loss_t = F.eb_aux_loss_grad(qd, pd, td, dq_t, loss_out=loss_in)
    assert loss_t is loss_in
    dq = dq_t.cpu().numpy()
    f64_gate(float(loss_t[0]), r["loss"], abs(r["loss32"] - r["loss"]) / r["loss"], f"eb_aux_loss_grad C={C} loss", floor=0.0)
    f64_gate(dq, r["dq"], close_ratio(r["dq32"], r["dq"], 0.1), f"eb_aux_loss_grad C={C} dq")
    dq0 = np.random.default_rng(8).uniform(-30.0, 30.0, (C, 1, 3)).astype(np.float32)
    acc = vec(dq0.copy())
    loss_a = F.eb_aux_loss_grad(qd, pd, td, acc, accumulate=True)
    assert np.array_equal(acc.cpu().numpy(), dq0 + dq) and torch.equal(loss_a, loss_t)
    loss_o, dq_o = F.eb_aux_loss(qd, pd, td)
    f64_gate(float(loss_o[0]), r["loss"], abs(r["loss32"] - r["loss"]) / r["loss"], f"eb_aux_loss C={C} loss", floor=0.0)
    f64_gate(dq_o.cpu().numpy(), r["dq"], close_ratio(r["dq32"], r["dq"], 0.1), f"eb_aux_loss C={C} dq")
    print(f"[aux kernels] C={C}: max |dq(block) - dq(256-thread)| = {np.abs(dq - dq_o.cpu().numpy()).max():.3e}   "
          f"|loss(block) - loss(256-thread)| = {abs(float(loss_t[0]) - float(loss_o[0])):.3e}")
    loss_n, dq_n = F.eb_aux_loss(qd, pd, td, need_grad=False)
    assert dq_n is None
    if C * 3 <= 256:                                                     # one workgroup: one atomic, the same bits without the gradient
        assert float(loss_n[0]) == float(loss_o[0])
    else:
        f64_gate(float(loss_n[0]), r["loss"], abs(r["loss32"] - r["loss"]) / r["loss"], f"eb_aux_loss C={C} loss, no gradient", floor=0.0)


def test_eb_aux_loss_grad_lds_attribute_is_kept(F):
    """C = 688 (the most one workgroup's LDS holds: 159 616 B dynamic + 4 096 B static), then C = 1, then 688 again: the cached
    dynamic-LDS attribute still admits the second large launch, which gives the bits of the first"""
    out = []
    for C in (er.AUX_MAX_C, 1, er.AUX_MAX_C):
        q, pack, target = er.aux_inputs(C)
        dq = torch.full((C, 1, 3), float("nan"), device="cuda")
        loss = F.eb_aux_loss_grad(vec(q), vec(pack), vec(target), dq)
        torch.cuda.synchronize()
        out.append((loss.clone(), dq))
    assert torch.equal(out[0][0], out[2][0]) and torch.equal(out[0][1], out[2][1]) and not torch.isnan(out[2][1]).any()
    r1 = er.aux_reference(1)
    f64_gate(out[1][1].cpu().numpy(), r1["dq"], close_ratio(r1["dq32"], r1["dq"], 0.1), "eb_aux_loss_grad C=1 after C=688 dq")


# =========================================================================================================== 3. eval-mode / explicit-noise forwards
@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_id)
def test_eb_forward_eval_and_noise_vs_float64(F, shape):
    """stem_eb_forward (per channel up to 4096 pixels, per element above): eval mode gives rint(z - median) + median in fp32 exactly,
    ties (median + k + 1/2, k even and odd, in every channel) to even; noise mode gives z + noise exactly; the likelihoods of both
    through f64_gate (atol 1e-9: the floor) against float64.  z is a channel slice of a wider buffer of NaNs."""
    B, H, W, C = shape
    pack = ref.eb_random_pack(C, 32)
    z, med = er.eb_eval_inputs(B, H, W, C, 33)
    _, noise = ref.eb_inputs(B, H, W, C, 33)
    zd, pd = nhwc(z, B, H, W, ld=C + 3, c0=1), vec(pack)
    assert F.nhwc_ld(zd) == C + 3
    for mode, kw, want in (("eval", {"medians": vec(med)}, er.round_about(z, med)), ("noise", {"noise": nhwc(noise, B, H, W)}, z + noise)):
        z_hat, lik = F.eb_forward(zd, pd, **kw)
        zh = flat(z_hat)
        assert np.array_equal(zh, want), mode
        exact = ref.eb_likelihood(zh, pack)
        assert (exact == 1e-9).mean() >= 0.02
        y32 = close_ratio(ref.eb_likelihood(zh, pack, torch.float32), exact, 0.1, 1e-9)
        f64_gate(flat(lik), exact, y32, f"eb_forward {mode} lik {_id(shape)}", atol=1e-9)
        if mode == "eval":
            assert np.array_equal(zh[:4] - med, np.repeat(np.array([-2.0, 2.0, 0.0, -0.0], np.float32)[:, None], C, axis=1))


@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_id)
def test_gc_forward_eval_vs_float64(F, shape):
    """stem_gc_forward in eval mode: out == rint(y - mean) + mean in fp32 exactly (every 13th element a tie), likelihoods through the
    gate of test_gc_forward_train_vs_float64; scales | means are channel slices of one 2C-wide buffer"""
    B, H, W, C = shape
    y, sc, mu = er.gc_eval_inputs(B, H, W, C, 43)
    gp = nhwc(np.concatenate([sc, mu], axis=1), B, H, W)
    out, lik = F.gc_forward(nhwc(y, B, H, W), gp[:, :C], gp[:, C:])
    o = flat(out)
    assert np.array_equal(o, er.round_about(y, mu))
    t = er.gc_tie_mask(B * H * W, C)
    assert ((o - mu)[t] % 2 == 0).all()
    exact = ref.gc_likelihood(o, sc, mu)
    assert (exact == 1e-9).mean() >= 0.04
    f64_gate(flat(lik), exact, close_ratio(ref.gc_likelihood(o, sc, mu, torch.float32), exact, 0.1, 1e-9), f"gc_forward eval lik {_id(shape)}", atol=1e-9)


@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_id)
def test_gc_backward_vs_float64(F, shape):
    """stand-alone stem_gc_backward with dy and a record, dlik = coef / lik: dscales, dmeans through f64_gate (atol 1e-9) against
    float64 autograd; dy == -dmeans exactly; below scale_bound the scale gradient passes only where it raises the scale; the record
    has one slot per 256 elements and bounds the gradients.  dscales | dmeans are slices of a 2C-wide buffer of NaNs."""
    B, H, W, C = shape
    n = B * H * W
    coef = -1.0 / (math.log(2.0) * n)
    y, noise, sc, mu = ref.gc_inputs(B, H, W, C, 41, tie=shape == ref.TAIL_SHAPES[0])
    o = y + noise
    dlik = (coef / ref.gc_likelihood(o, sc, mu)).astype(np.float32)
    gp = nhwc(np.concatenate([sc, mu], axis=1), B, H, W)
    dgp = nhwc(np.full((n, 2 * C), np.nan, np.float32), B, H, W)
    dy = nhwc(np.full((n, C), np.nan, np.float32), B, H, W)
    q = F.gc_backward(nhwc(o, B, H, W), gp[:, :C], gp[:, C:], nhwc(dlik, B, H, W), dgp[:, :C], dgp[:, C:], dy=dy, record=True)
    ds, dm = flat(dgp[:, :C]), flat(dgp[:, C:])
    ds64, dm64 = ref.gc_backward(o, sc, mu, coef)
    ds32, dm32 = ref.gc_backward(o, sc, mu, coef, torch.float32)
    what = f"gc_backward {_id(shape)}"
    f64_gate(ds, ds64, close_ratio(ds32, ds64, 0.1, 1e-9), what + " dscales", atol=1e-9)
    f64_gate(dm, dm64, close_ratio(dm32, dm64, 0.1, 1e-9), what + " dmeans", atol=1e-9)
    assert np.array_equal(flat(dy), -dm)
    low = sc < 0.11
    assert (ds[low] <= 0).all() and (ds[low] < 0).any() and (ds[low] == 0).any()
    ns, rmax = rec_max(q)
    assert ns == (n * C + 255) // 256 and rmax >= float(max(np.abs(ds).max(), np.abs(dm).max()))
    # without dy and record: the same gradients
    dgp2 = nhwc(np.full((n, 2 * C), np.nan, np.float32), B, H, W)
    assert F.gc_backward(nhwc(o, B, H, W), gp[:, :C], gp[:, C:], nhwc(dlik, B, H, W), dgp2[:, :C], dgp2[:, C:]) is None
    assert torch.equal(dgp2, dgp)


# =========================================================================================================== 4. build_indexes
@pytest.mark.parametrize("ld", [None, er.INDEX_SHAPE[3] + 3], ids=["dense", "slice"])
def test_build_indexes_at_the_table_entries(F, golden, ld):
    """scales at, just above and just below every entry of the golden scale table (s <= table[t] decides the symbol table), 0, the
    scale bound and its neighbours, a scale above the table: equal to the C oracle and to the searchsorted statement; dense and as a
    channel slice of a wider buffer"""
    table = golden("codec.npz")["gc:scale_table"]
    s = er.index_scales(table)
    B, H, W, C = er.INDEX_SHAPE
    sd = nhwc(s, B, H, W) if ld is None else nhwc(s, B, H, W, ld=ld, c0=2)
    idx = F.build_indexes(sd, vec(table))
    got = idx.permute(0, 2, 3, 1).contiguous().reshape(-1, C).cpu().numpy()
    assert got.dtype == np.int32
    assert np.array_equal(got, orc.build_indexes(s, table)) and np.array_equal(got, er.build_indexes(s, table))


# =========================================================================================================== 5. log2 sum, dlog, pack / unpack
@pytest.mark.parametrize("n", er.LOG2_SIZES)
def test_log2_sum_grid_stride_and_accumulator(F, n):
    """acc += sum log2(lik) beyond the 1024 x 256 elements one trip of the grid covers, into an accumulator that holds a value: each
    term is one rounded log2f, so |sum - exact| <= n * 2^-23 * max |log2 lik| (the bound of _check_rate_outputs)"""
    lik = er.log2_likelihoods()[:n]
    acc0 = -4096.5
    acc = torch.full((1,), acc0, dtype=torch.float64, device="cuda")
    F.log2_sum(vec(lik), acc)
    lg = np.log2(lik.astype(np.float64))
    exact = math.fsum(lg)
    bound = n * 2.0 ** -23 * float(np.abs(lg).max())
    got = float(acc[0]) - acc0
    print(f"[log2 sum] n={n}: |sum - exact| = {abs(got - exact):.3e}   bound n * 2^-23 * max|log2 lik| = {bound:.3e}")
    assert abs(got - exact) <= bound


def test_dlog_257(F):
    lik = er.log2_likelihoods()[:257]
    got = F.dlog(vec(lik), -0.37).cpu().numpy()
    assert_close(got, np.float32(-0.37).astype(np.float64) / lik.astype(np.float64), rtol=1e-6, what="dlog", floor=0.0)


@pytest.mark.parametrize("C", [1, 5, 320])
def test_eb_pack_and_unpack(F, C):
    """eb_pack == orc.eb_pack_params and eb_unpack_grads == orc.eb_unpack_grads, exactly (copies); accumulate=True adds in one fp32 add"""
    rng = np.random.default_rng(100 + C)
    sd = {"entropy_bottleneck." + n: rng.standard_normal((C, *s)).astype(np.float32) for n, s in zip(ref.EB_NAMES, ref.EB_SHAPES)}
    assert F.EB_TENSORS == ref.EB_NAMES
    pack = F.eb_pack([vec(sd["entropy_bottleneck." + n]) for n in F.EB_TENSORS])
    assert np.array_equal(pack.cpu().numpy(), orc.eb_pack_params(sd))
    dpack = rng.standard_normal((C, 58)).astype(np.float32)
    want = orc.eb_unpack_grads(dpack)
    grads = [torch.full((C, *s), float("nan"), device="cuda") for s in ref.EB_SHAPES]
    F.eb_unpack_grads(vec(dpack), grads)
    for n, g in zip(F.EB_TENSORS, grads):
        assert np.array_equal(g.cpu().numpy(), want["entropy_bottleneck." + n]), n
    old = [rng.standard_normal((C, *s)).astype(np.float32) for s in ref.EB_SHAPES]
    grads = [vec(o.copy()) for o in old]
    F.eb_unpack_grads(vec(dpack), grads, accumulate=True)
    for n, g, o in zip(F.EB_TENSORS, grads, old):
        assert np.array_equal(g.cpu().numpy(), o + want["entropy_bottleneck." + n]), n
