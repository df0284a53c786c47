"""GPU parity tests, op level, for the tail of the training step: the kernels that turn the network's outputs into a loss, a gradient
norm and a parameter update (noise stream, prior prologue, fused likelihood / rate kernels, loss reductions, sumsq / clip / Adam).

Each kernel is called on its own and compared with a plain reference of the same operation (tests/train_tail_ref.py, pinned on the
CPU by tests/test_train_tail_ref.py): bit for bit where the operation is exact (Philox words, adds, copies, rounding to integers,
maxima), through conftest.f64_gate at the project's 1e-4 against float64 where it is fp32 arithmetic, and with bounds derived from
the arithmetic (stated at each site) for the reductions."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import train_tail_ref as ref
from conftest import REPO, assert_close, close_ratio, f64_gate

sys.path.insert(0, os.path.join(REPO, "oracle"))
import stem_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SEED_HI = (0xA4093822 << 32) | 0x299F31D0          # a seed with bits above 2^32: the second key word is not zero
U24, U53 = 2.0 ** -24, 2.0 ** -53


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return functional


def nhwc(a, B, H, W, ld=None, c0=0, fill=float("nan")):
    """[npix, C] numpy -> [B,C,H,W] device tensor with NHWC memory; ld: as channels c0 .. c0 + C of a buffer ld channels wide (the
    other channels hold `fill`)"""
    a = np.ascontiguousarray(a, np.float32)
    C = a.shape[1]
    if ld is None:
        return torch.from_numpy(a.reshape(B, H, W, C)).cuda().permute(0, 3, 1, 2)
    buf = torch.full((B, H, W, ld), fill, dtype=torch.float32, device="cuda")
    buf[..., c0:c0 + C] = torch.from_numpy(a.reshape(B, H, W, C)).cuda()
    return buf.permute(0, 3, 1, 2)[:, c0:c0 + C]


def flat(t):
    """[B,C,H,W] device tensor (any layout, channel slices included) -> [npix, C] numpy"""
    return t.detach().permute(0, 2, 3, 1).contiguous().reshape(-1, t.shape[1]).cpu().numpy()


def vec(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rec_max(q):
    """a producer's scale record (stem_common.h: slot count, 2^-e, 14 reserved words, one max |value| per workgroup) -> (slots, max)"""
    q = q.cpu()
    ns = int(q[:1].view(torch.int32)[0])
    assert 0 < ns <= q.numel() - 16
    return ns, float(q[16:16 + ns].max())


# =========================================================================================================== 1. noise stream
def test_uniform_noise_is_philox4x32_10(F):
    """stem_uniform_noise == Philox4x32-10 with counter (offset + q, 0, 0) and key (seed_lo, seed_hi), bit for bit: sizes around the
    4-value block and the 256-thread workgroup, a 64-bit seed, a carry of the low counter word inside the tensor and a wrap at 2^64"""
    for n in (1, 3, 4, 1021, 4 * 256 + 1):
        like = F.empty_nhwc(1, n, 1, 1, "cuda")
        for seed, offset in ((1234, 0), (SEED_HI, 2 ** 32 - 2), (SEED_HI + 1, 2 ** 64 - 3), (7, 2 ** 40 + 5)):
            got = F.uniform_noise_like(like, seed, offset).cpu().numpy().reshape(-1)
            assert np.array_equal(got, ref.philox_uniform(n, seed, offset)), (n, hex(seed), hex(offset))


@pytest.mark.parametrize("e", [0, 3])
def test_uniform_noise_epoch_advances_by_2_40(F, e):
    """the device-resident epoch adds e * 2^40 to the counter (what replays of a captured graph rely on)"""
    epoch = torch.tensor(e, dtype=torch.int64, device="cuda")
    for n, offset in ((1021, 2 ** 32 - 2), (5, 2 ** 64 - 2 ** 41 - 1)):
        got = F.uniform_noise_like(F.empty_nhwc(1, n, 1, 1, "cuda"), SEED_HI, offset, epoch=epoch).cpu().numpy().reshape(-1)
        assert np.array_equal(got, ref.philox_uniform(n, SEED_HI, offset + e * 2 ** 40))
        assert np.array_equal(got, ref.philox_uniform(n, SEED_HI, offset, epoch=e))


def _tail_id(s):
    return "B%d_%dx%d_C%d" % s


@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_tail_id)
def test_fused_kernels_draw_the_noise_stream(F, shape):
    """eb_forward_train (both kernels: <= 4096 pixels per channel and above) and gc_forward_train with noise=None add the values
    stem_uniform_noise gives for the dense NHWC index i: counter offset [+ epoch * 2^40] + (i >> 2), word i & 3.  C = 3 / 5: the word
    does not line up with the channel."""
    B, H, W, C = shape
    n = B * H * W
    z, _ = ref.eb_inputs(B, H, W, C, 11)
    pack = vec(ref.eb_random_pack(C, 12))
    epoch = torch.tensor(3, dtype=torch.int64, device="cuda")
    for seed, offset, ep in ((SEED_HI, 2 ** 32 - 2, None), (99, 17, epoch)):
        r = ref.philox_uniform(n * C, seed, offset, epoch=0 if ep is None else 3).reshape(n, C)
        z_hat = F.eb_forward_train(nhwc(z, B, H, W, ld=C + 3, c0=2), pack, -0.01, seed=seed, offset=offset, epoch=ep)[0]
        assert np.array_equal(flat(z_hat), z + r), "eb_forward_train"
        y, _, sc, mu = ref.gc_inputs(B, H, W, C, 13)
        out = F.gc_forward_train(nhwc(y, B, H, W), nhwc(sc, B, H, W), nhwc(mu, B, H, W), -0.01, seed=seed, offset=offset, epoch=ep)[0]
        assert np.array_equal(flat(out), y + r), "gc_forward_train"


# =========================================================================================================== 2. prior_prologue
PP = (2, 9, 11, 12)          # 198 pixels x 3 four-channel groups = 594 threads: two full workgroups and a partial one
HALVES = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5], np.float32)


def _pp_inputs(B, H, W, C, seed):
    rng = np.random.default_rng(seed)
    n = B * H * W
    yd = (np.round(rng.uniform(-6, 6, (n, C)) * 4) / 4).astype(np.float32)
    yc = rng.uniform(-6, 6, (n, C)).astype(np.float32)
    # ties of the rounding, in both modes: target = yc (yd = 0) in the first pixel's first six channels, yc - yd in the next six
    yd[0, :6], yc[0, :6] = 0.0, HALVES
    yc[0, 6:12] = yd[0, 6:12] + HALVES
    yc[n - 1, :6] = yd[n - 1, :6] + HALVES[::-1]
    return yc, yd


def _pp_reference(yc, yd, residual, training, r):
    target = (yc - yd) if residual else yc.copy()
    t_hat = (target + r) if training else np.rint(target)
    y_hat = (t_hat + yd) if residual else t_hat.copy()
    return np.concatenate([yc, yd], axis=1), target, t_hat.astype(np.float32), y_hat.astype(np.float32)


@pytest.mark.parametrize("with_t_hat", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("residual", [True, False])
def test_prior_prologue(F, residual, training, with_t_hat):
    """he_in = [y_cur | y_cond], target = y_cur - y_cond | y_cur, t_hat = target + noise | round-half-even(target), y_hat = t_hat
    (+ y_cond): all exact in fp32, against numpy.  Inputs are channel slices of wider buffers (pitches 20 and 16 for C = 12); noise
    once as an explicit tensor and once drawn in the kernel (counter = the 4-channel group's index); the scale records hold the
    maxima of he_in and t_hat."""
    B, H, W, C = PP
    n = B * H * W
    yc, yd = _pp_inputs(B, H, W, C, 21)
    ycd, ydd = nhwc(yc, B, H, W, ld=20, c0=4), nhwc(yd, B, H, W, ld=16, c0=0)
    assert F.nhwc_ld(ycd) == 20 and F.nhwc_ld(ydd) == 16
    explicit = np.random.default_rng(22).uniform(-0.5, 0.5, (n, C)).astype(np.float32)
    epoch = torch.tensor(3, dtype=torch.int64, device="cuda")
    for kw, r in (({"noise": nhwc(explicit, B, H, W)}, explicit),
                  ({"seed": SEED_HI, "offset": 2 ** 32 - 100}, ref.philox_uniform(n * C, SEED_HI, 2 ** 32 - 100).reshape(n, C)),
                  ({"seed": 5, "offset": 9, "epoch": epoch}, ref.philox_uniform(n * C, 5, 9, epoch=3).reshape(n, C))):
        records = {}
        he_in, target, t_hat, y_hat = F.prior_prologue(ycd, ydd, residual, training, with_t_hat, records=records, **kw)
        e_in, e_target, e_t, e_y = _pp_reference(yc, yd, residual, training, r)
        assert np.array_equal(flat(he_in), e_in) and np.array_equal(flat(target), e_target)
        assert rec_max(records["in"]) == ((n * C // 4 + 255) // 256, float(np.abs(e_in).max()))
        if not with_t_hat:
            assert t_hat is None and y_hat is None and "t_hat" not in records
            continue
        assert np.array_equal(flat(t_hat), e_t) and np.array_equal(flat(y_hat), e_y)
        assert rec_max(records["t_hat"]) == ((n * C // 4 + 255) // 256, float(np.abs(e_t).max()))
        if not training:
            assert np.array_equal(flat(t_hat)[0, :6], [0.0, -0.0, 2.0, -2.0, 2.0, -2.0])           # half to even


def test_prior_prologue_records_feed_the_fp16_split(F):
    """the maxima F16Planes.split(..., src_q=) takes from the "in" and "t_hat" records are max |he_in| and max |t_hat| exactly (C = 32:
    the planes layout needs 32-channel slabs)"""
    B, H, W, C = 2, 9, 11, 32
    yc, yd = _pp_inputs(B, H, W, C, 23)
    yc[100, 7] = -37.25                                      # the maximum sits in one workgroup's slot only
    records = {}
    he_in, _, t_hat, _ = F.prior_prologue(nhwc(yc, B, H, W, ld=40, c0=8), nhwc(yd, B, H, W), True, True, True, seed=3, offset=4,
                                          records=records)
    assert F.F16Planes.split(he_in, src_q=records["in"].data_ptr()).record()[1] == float(np.abs(flat(he_in)).max()) == 37.25
    assert F.F16Planes.split(t_hat, src_q=records["t_hat"].data_ptr()).record()[1] == float(np.abs(flat(t_hat)).max())


# =========================================================================================================== 3. fused likelihood / rate / gradient kernels
def _check_rate_outputs(F, lik, dlik, part, coef, what):
    """dlik == coef / lik to 1e-6 of the device's own lik (the bound stem_dlog has); one partial per workgroup; their sum against the
    float64 sum of log2 of the device's lik: each term is one rounded log2f, i.e. off by at most 2^-23 |log2 lik|, and the double
    accumulation adds nothing visible, so |sum - exact| <= n * 2^-23 * max |log2 lik|"""
    lik64 = lik.astype(np.float64)
    assert_close(dlik, coef / lik64, rtol=1e-6, what=what + " dlik", floor=0.0)
    assert part.numel() == F.rate_partials(lik.size) == (lik.size + 255) // 256
    exact = math.fsum(np.log2(lik64).ravel())
    got = math.fsum(part.cpu().numpy())
    bound = lik.size * 2.0 ** -23 * float(np.abs(np.log2(lik64)).max())
    print(f"[rate sum] {what}: |sum - exact| = {abs(got - exact):.3e}   bound n * 2^-23 * max|log2 lik| = {bound:.3e}")
    assert abs(got - exact) <= bound, f"{what}: sum of the log2 partials {got!r} vs {exact!r}"


@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_tail_id)
def test_eb_forward_train_vs_float64(F, shape):
    """EntropyBottleneck training forward with explicit noise: z_hat exact, likelihoods gated against float64 (atol 1e-9: the floor),
    dlik, rate partials, and the z_hat record (= max |z_hat|, for the fp16 split in front of the hyper decoder); z is a channel slice.
    Both kernels (per channel up to 4096 pixels, per element above) run over the shapes."""
    B, H, W, C = shape
    coef = -1.0 / (math.log(2.0) * B * H * W)
    z, noise = ref.eb_inputs(B, H, W, C, 31)
    pack = ref.eb_random_pack(C, 32)
    zd, nd, pd = nhwc(z, B, H, W, ld=C + 3, c0=1), nhwc(noise, B, H, W), vec(pack)
    z_hat, lik, dlik, part, q = F.eb_forward_train(zd, pd, coef, noise=nd, record=True)
    zh = flat(z_hat)
    assert np.array_equal(zh, z + noise)
    exact = ref.eb_likelihood(zh, pack)
    y32 = close_ratio(ref.eb_likelihood(zh, pack, torch.float32), exact, 0.1, 1e-9)
    assert (exact == 1e-9).sum() >= zh.size // 40                      # the inputs reach the floor (every 16th is far out; not every tail is that thin)
    f64_gate(flat(lik), exact, y32, f"eb_forward_train lik {_tail_id(shape)}", atol=1e-9)
    _check_rate_outputs(F, flat(lik), flat(dlik), part, coef, f"eb_forward_train {_tail_id(shape)}")
    assert rec_max(q) == ((zh.size + 255) // 256, float(np.abs(zh).max()))
    plain = F.eb_forward_train(zd, pd, coef, noise=nd)
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, (z_hat, lik, dlik, part)))


@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_tail_id)
def test_gc_forward_train_vs_float64(F, shape):
    """GaussianConditional training forward with its backward folded in: out exact, likelihoods / dscales / dmeans gated against
    float64 with the gates of test_gaussian_conditional_golden (1e-4, atol 1e-9, floor 0.1).  scales | means and dscales | dmeans are
    channel slices of 2C-wide buffers; a quarter of the scales lie below scale_bound (their gradient passes only where it raises the
    scale), every 16th likelihood is at the 1e-9 floor.  The record is >= max(|dscales|, |dmeans|), == when no out equals its mean."""
    B, H, W, C = shape
    tie = shape == ref.TAIL_SHAPES[0]
    coef = -1.0 / (math.log(2.0) * B * H * W)
    y, noise, sc, mu = ref.gc_inputs(B, H, W, C, 41, tie=tie)
    gp = nhwc(np.concatenate([sc, mu], axis=1), B, H, W)
    dgp = nhwc(np.full((B * H * W, 2 * C), np.nan, np.float32), B, H, W)
    yd, nd = nhwc(y, B, H, W), nhwc(noise, B, H, W)
    out, lik, dlik, part, q = F.gc_forward_train(yd, gp[:, :C], gp[:, C:], coef, noise=nd, backward=(dgp[:, :C], dgp[:, C:]), record=True)
    o = flat(out)
    assert np.array_equal(o, y + noise) and bool((o == mu).any()) == tie
    exact = ref.gc_likelihood(o, sc, mu)
    assert (exact == 1e-9).sum() >= o.size // 20
    what = f"gc_forward_train {_tail_id(shape)}"
    f64_gate(flat(lik), exact, close_ratio(ref.gc_likelihood(o, sc, mu, torch.float32), exact, 0.1, 1e-9), what + " lik", atol=1e-9)
    _check_rate_outputs(F, flat(lik), flat(dlik), part, coef, what)
    ds64, dm64 = ref.gc_backward(o, sc, mu, coef)
    ds32, dm32 = ref.gc_backward(o, sc, mu, coef, torch.float32)
    ds, dm = flat(dgp[:, :C]), flat(dgp[:, C:])
    f64_gate(ds, ds64, close_ratio(ds32, ds64, 0.1, 1e-9), what + " dscales", atol=1e-9)
    f64_gate(dm, dm64, close_ratio(dm32, dm64, 0.1, 1e-9), what + " dmeans", atol=1e-9)
    low = sc < 0.11
    assert (ds[low] <= 0).all() and (ds[low] < 0).any() and (ds[low] == 0).any()
    ns, rmax = rec_max(q)
    gmax = float(max(np.abs(ds).max(), np.abs(dm).max()))
    assert ns == (o.size + 255) // 256 and rmax >= gmax and (tie or rmax == gmax)
    plain = F.gc_forward_train(yd, gp[:, :C], gp[:, C:], coef, noise=nd)
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, (out, lik, dlik, part)))


def bits(t):
    """flat(t) as int32: what "bit-identical" compares (-0.0 differs from +0.0, a NaN equals itself)"""
    return flat(t).view(np.int32)


@pytest.mark.parametrize("shape", [ref.TAIL_SHAPES[0], ref.TAIL_SHAPES[3]], ids=_tail_id)
def test_gc_fused_backward_is_the_stand_alone_backward(F, shape):
    """the backward that gc_forward_train folds in and gc_backward run on the fused call's own out and dlik are one element function
    (csrc/entropy_elem.h: gauss_bwd_elem): dscales, dmeans and the whole scale record bit for bit.  The inputs of
    test_gc_forward_train_vs_float64: a partial last workgroup, a quarter of the scales below the bound, likelihoods at the floor, and
    out == mean in the first shape."""
    B, H, W, C = shape
    n = B * H * W
    tie = shape == ref.TAIL_SHAPES[0]
    coef = -1.0 / (math.log(2.0) * n)
    y, noise, sc, mu = ref.gc_inputs(B, H, W, C, 41, tie=tie)
    assert (n * C) % 256 != 0 and (sc < 0.11).mean() > 0.2
    gp = nhwc(np.concatenate([sc, mu], axis=1), B, H, W)
    fused, alone = (nhwc(np.full((n, 2 * C), np.nan, np.float32), B, H, W) for _ in range(2))
    out, lik, dlik, _, q = F.gc_forward_train(nhwc(y, B, H, W), gp[:, :C], gp[:, C:], coef, noise=nhwc(noise, B, H, W),
                                              backward=(fused[:, :C], fused[:, C:]), record=True)
    assert (flat(lik) == np.float32(1e-9)).sum() >= n * C // 20 and bool((flat(out) == mu).any()) == tie
    q_alone = F.gc_backward(out, gp[:, :C], gp[:, C:], dlik, alone[:, :C], alone[:, C:], record=True)
    assert not np.isnan(flat(fused)).any()
    assert np.array_equal(bits(fused[:, :C]), bits(alone[:, :C])), "dscales"
    assert np.array_equal(bits(fused[:, C:]), bits(alone[:, C:])), "dmeans"
    assert q.numel() == q_alone.numel() == 16 + (n * C + 255) // 256
    assert torch.equal(q.view(torch.int32), q_alone.view(torch.int32)), "scale record"


EB_CM_MAX_PIX = 4096         # stem_eb_forward / stem_eb_forward_train: up to this many pixels the one-workgroup-per-channel kernel runs


@pytest.mark.parametrize("shape", [ref.TAIL_SHAPES[0], ref.TAIL_SHAPES[2]], ids=_tail_id)
def test_eval_and_train_likelihoods_are_one_expression(F, shape):
    """gc_forward and eb_forward in noise mode with an explicit tensor against gc_forward_train / eb_forward_train fed the same
    tensor: the quantised values and the likelihoods bit for bit.  198 and 4160 pixels per channel: the per-channel and the
    per-element kernel of each bottleneck pair."""
    small, large = (s[0] * s[1] * s[2] for s in (ref.TAIL_SHAPES[0], ref.TAIL_SHAPES[2]))
    assert small <= EB_CM_MAX_PIX < large
    B, H, W, C = shape
    coef = -1.0 / (math.log(2.0) * B * H * W)
    y, noise, sc, mu = ref.gc_inputs(B, H, W, C, 41)
    gp = nhwc(np.concatenate([sc, mu], axis=1), B, H, W)
    yd, nd = nhwc(y, B, H, W), nhwc(noise, B, H, W)
    out_e, lik_e = F.gc_forward(yd, gp[:, :C], gp[:, C:], noise=nd)
    out_t, lik_t = F.gc_forward_train(yd, gp[:, :C], gp[:, C:], coef, noise=nd)[:2]
    assert np.array_equal(bits(out_e), bits(out_t)) and np.array_equal(bits(lik_e), bits(lik_t)), "gc"
    assert (flat(lik_e) == np.float32(1e-9)).any() and (flat(lik_e) > np.float32(1e-9)).any()
    z, znoise = ref.eb_inputs(B, H, W, C, 31)
    zd, znd, pd = nhwc(z, B, H, W, ld=C + 3, c0=1), nhwc(znoise, B, H, W), vec(ref.eb_random_pack(C, 32))
    zhat_e, zlik_e = F.eb_forward(zd, pd, noise=znd)
    zhat_t, zlik_t = F.eb_forward_train(zd, pd, coef, noise=znd)[:2]
    assert np.array_equal(bits(zhat_e), bits(zhat_t)) and np.array_equal(bits(zlik_e), bits(zlik_t)), "eb"
    assert (flat(zlik_e) == np.float32(1e-9)).any() and (flat(zlik_e) > np.float32(1e-9)).any()


# =========================================================================================================== 4. loss reductions
def test_em_loss_finalize(F):
    """out = scale * (sum py, sum pz, both), double: against exactly rounded sums.  Any summation order of n doubles is within
    (n - 1) * 2^-53 of the exact sum relative to the sum of absolute values, the scaling adds one rounding: bound (ny + nz) * 2^-53
    of scale * sum |p|.  Sizes around the 256-thread workgroup, empty lists, a negative scale; out[2] == out[0] + out[1] exactly."""
    rng = np.random.default_rng(51)
    scale = -1.0 / 1234.5
    sizes = (0, 1, 255, 256, 257, 1000)
    for ny, nz in [(a, b) for a in sizes for b in sizes if a in (0, 257) or b in (0, 1000) or a == b]:
        py, pz = rng.uniform(-3000.0, 100.0, ny), rng.uniform(-900.0, 30.0, nz)
        out = F.em_loss_finalize(vec(py), vec(pz), scale).cpu().numpy()
        bound = (ny + nz) * U53 * abs(scale) * (np.abs(py).sum() + np.abs(pz).sum())
        assert abs(out[0] - math.fsum(py) * scale) <= bound and abs(out[1] - math.fsum(pz) * scale) <= bound, (ny, nz, out)
        assert out[2] == out[0] + out[1] and (ny or out[0] == 0.0) and (nz or out[1] == 0.0)
    into = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    assert F.em_loss_finalize(vec(py), vec(pz), scale, out3=into) is into and np.array_equal(into.cpu().numpy(), out)


SQERR_SHAPES = [(2, 3, 1, 1), (2, 3, 5, 7), (2, 3, 33, 31), (1, 3, 300, 300)]       # the last: 270000 elements > 1024 x 256, the grid-stride loop


def _sqerr_inputs(B, C, H, W, seed):
    """NCHW images and a non-constant weight map [B,1,H,W]; the map is the head of a four times larger buffer of NaNs, so an index that
    runs past the map shows instead of reading a neighbour's memory"""
    rng = np.random.default_rng(seed)
    xhat, x = rng.uniform(0, 1, (B, C, H, W)).astype(np.float32), rng.uniform(0, 1, (B, C, H, W)).astype(np.float32)
    lam = rng.uniform(0.25, 4.0, (B, 1, H, W)).astype(np.float32)
    buf = torch.full((4 * lam.size,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:lam.size] = vec(lam.reshape(-1))
    return xhat, x, lam, buf[:lam.size].view(B, 1, H, W)


@pytest.mark.parametrize("shape", SQERR_SHAPES, ids=lambda s: "B%d_C%d_%dx%d" % s)
def test_weighted_sqerr_sum_and_bwd(F, shape):
    """sum lam (xhat - x)^2 over NCHW with lam [B,1,H,W], fp64 accumulation of fp32 terms.  A term is fl(lam * fl(d * d)) with
    d = fl(xhat - x): d is off by 2^-24 (2^-23 in its square), each product by 2^-24, so every term, and with it the sum of these
    non-negative terms, is within 4 * 2^-24 = 2 * 2^-23 of exact: the gate, derived, not fitted.
    The backward g * coef * 2 * lam * (xhat - x) is a handful of fp32 roundings of known inputs: 1e-6, element-wise."""
    B, C, H, W = shape
    xhat, x, lam, lamd = _sqerr_inputs(B, C, H, W, 61)
    xd, xh = vec(x), vec(xhat)
    exact = math.fsum((lam.astype(np.float64) * (xhat.astype(np.float64) - x) ** 2).ravel())
    got = float(F.weighted_sqerr_sum(xh, xd, lamd))
    print(f"[sqerr sum] {shape}: relative error {abs(got - exact) / exact:.3e}   bound {2 * 2.0 ** -23:.3e}")
    assert abs(got - exact) <= 2 * 2.0 ** -23 * exact
    g, coef = torch.tensor(-1.75 * 255 ** 2, dtype=torch.float64, device="cuda"), 1.0 / x.size
    want = float(g) * float(np.float32(coef)) * 2.0 * lam.astype(np.float64) * (xhat.astype(np.float64) - x)
    assert_close(F.weighted_sqerr_bwd(xh, xd, lamd, g, coef).cpu().numpy(), want, rtol=1e-6, what="weighted_sqerr_bwd", floor=0.0)


def test_rate_distortion_loss_mse_vs_float64(F):
    """losses.RateDistortionLoss(metric="mse") on tiny tensors against float64 torch on the CPU: the distortion through the gate of
    weighted_sqerr_sum, the rate through the log2-sum bound, the total exactly the combination of the two, x_hat.grad at 1e-6"""
    from spatiotemporalentropymodel_amd.losses import RateDistortionLoss
    B, C, H, W, lmbda = 2, 3, 4, 5, 0.0130
    rng = np.random.default_rng(71)
    xhat, x = rng.uniform(0, 1, (B, C, H, W)).astype(np.float32), rng.uniform(0, 1, (B, C, H, W)).astype(np.float32)
    liks = {"y": rng.uniform(1e-9, 1.0, (B, 8, 2, 3)).astype(np.float32), "z": rng.uniform(1e-4, 1.0, (B, 4, 1, 2)).astype(np.float32)}
    xh = vec(xhat).requires_grad_(True)
    out = RateDistortionLoss(lmbda=lmbda)({"x_hat": xh, "likelihoods": {k: vec(v) for k, v in liks.items()}}, vec(x))
    out["loss"].backward()
    t = torch.from_numpy(xhat).double().requires_grad_(True)
    mse = ((t - torch.from_numpy(x).double()) ** 2).mean()
    bpp = sum(torch.log2(torch.from_numpy(v).double()).sum() / (-B * H * W) for v in liks.values())
    (lmbda * 255 ** 2 * mse + bpp).backward()
    assert abs(float(out["mse_loss"]) - float(mse)) <= 2 * 2.0 ** -23 * float(mse)
    nlik = sum(v.size for v in liks.values())
    assert abs(float(out["bpp_loss"]) - float(bpp)) <= nlik * 2.0 ** -23 * math.log2(1e9) / (B * H * W)
    assert abs(float(out["loss"]) - (lmbda * 255 ** 2 * float(out["mse_loss"]) + float(out["bpp_loss"]))) <= 4 * U53 * abs(float(out["loss"]))
    assert out["loss"].dtype == torch.float64
    assert_close(xh.grad.cpu().numpy(), t.grad.numpy(), rtol=1e-6, what="RateDistortionLoss d x_hat", floor=0.0)


# =========================================================================================================== 5. norm, clip, Adam
@pytest.fixture(scope="module")
def grad_2m():
    """the largest tensor of this file: 4 * 256 * 2048 + 7 floats, so that the grid is capped at STEM_SUMSQ_SCRATCH workgroups (every
    workgroup loops) and a tail of 7 is left for the scalar loop"""
    return np.random.default_rng(81).standard_normal(4 * 256 * 2048 + 7 + 1).astype(np.float32)


@pytest.mark.parametrize("n", [1, 3, 1023, 4 * 256 * 2048 + 7])
def test_sumsq_vs_float64(F, grad_2m, n):
    """sum g^2 accumulated in double: the squares of floats are exact in double, so only the summation rounds, at most (n - 1) * 2^-53
    relative for any order: bound n * 2^-53 against the exactly rounded sum.  Aligned (vector route + tail) and from a view that
    starts 4 bytes into the buffer (scalar route); bit-reproducible; overwrite=True ignores what the accumulator held."""
    buf = vec(grad_2m)
    for g, gn in ((buf[:n], grad_2m[:n]), (buf[1:n + 1], grad_2m[1:n + 1])):
        exact = math.fsum(gn.astype(np.float64) ** 2)
        acc, acc2 = F.sumsq_accumulator("cuda"), F.sumsq_accumulator("cuda")
        F.sumsq(g, acc)
        F.sumsq(g, acc2)
        assert abs(float(acc[0]) - exact) <= n * U53 * exact, (n, float(acc[0]), exact)
        assert float(acc[0]) == float(acc2[0])
        junk = torch.full((1 + F.SUMSQ_SCRATCH,), float("nan"), dtype=torch.float64, device="cuda")
        F.sumsq(g, junk, overwrite=True)
        assert float(junk[0]) == float(acc[0])
        F.sumsq(g, acc)                                                     # accumulates: acc[0] + the same sum, one rounding
        assert float(acc[0]) == 2.0 * float(acc2[0])
    assert buf[1:].data_ptr() % 16 == 4 and buf.data_ptr() % 16 == 0


def test_clip_scale(F):
    """clip_grad_norm_ on its own: below max_norm the gradient is untouched bit for bit; above it g <- fl(g * coef), coef =
    max_norm / (norm + 1e-6) from the float64 norm, element-wise to 1e-6 (the coefficient is formed in fp32)"""
    g0 = np.random.default_rng(82).standard_normal(3 * 256 + 77).astype(np.float32)
    g0[5] = 0.0
    norm = math.sqrt(math.fsum(g0.astype(np.float64) ** 2))
    for max_norm in (float(np.float32(1.0001 * norm + 1e-5)), 2.0 * norm, 1.0, 0.25 * norm):
        g, acc = vec(g0.copy()), F.sumsq_accumulator("cuda")
        F.sumsq(g, acc)
        F.clip_scale(g, acc, max_norm)
        if max_norm > norm:
            assert np.array_equal(g.cpu().numpy(), g0)
        else:
            assert_close(g.cpu().numpy(), g0.astype(np.float64) * (max_norm / (norm + 1e-6)), rtol=1e-6, what="clip_scale", floor=0.0)
            assert float(g[5]) == 0.0


def test_axpy_and_lrelu_exact(F):
    """y += a * x and LeakyReLU forward / backward on sizes that are no multiple of the workgroup.  x, y are multiples of 2^-20 in
    [-1, 1] and a one of 2^-10, so a * x + y is exact in double: the kernel must give either fl(fl(a * x) + y) or, where the compiler
    contracts the expression, the fused fl(a * x + y) -- the same form for every element (the two differ by at most one ulp; the
    build at hand contracts).  lrelu: x > 0 ? x : x * slope, one rounding, against the oracle's."""
    rng = np.random.default_rng(83)
    n = 4 * 256 + 131
    x, y = (rng.integers(-2 ** 20, 2 ** 20, n) * 2.0 ** -20).astype(np.float32), (rng.integers(-2 ** 20, 2 ** 20, n) * 2.0 ** -20).astype(np.float32)
    a = 379 * 2.0 ** -10
    got = F.axpy_(vec(y.copy()), vec(x), a).cpu().numpy()
    plain = (np.float32(a) * x).astype(np.float32) + y
    fused = (a * x.astype(np.float64) + y.astype(np.float64)).astype(np.float32)
    assert (plain != fused).any() and np.abs(plain.astype(np.float64) - fused).max() <= np.spacing(np.float32(2.0))
    form = "fused" if np.array_equal(got, fused) else "separate"
    print(f"[axpy] multiply-add form of this build: {form}")
    assert np.array_equal(got, fused) or np.array_equal(got, plain)
    B, C, H, W = 1, 7, 11, 17                                     # 1309 elements
    v, dy = rng.standard_normal((B * H * W, C)).astype(np.float32), rng.standard_normal((B * H * W, C)).astype(np.float32)
    v[3, 2] = 0.0
    for slope in (0.01, 0.2):
        fwd = flat(F.lrelu_fwd(nhwc(v, B, H, W), slope))
        assert np.array_equal(fwd, orc.lrelu_fwd(v, slope)) and np.array_equal(fwd, np.where(v > 0, v, v * np.float32(slope)))
        bwd = flat(F.lrelu_bwd(nhwc(fwd, B, H, W), nhwc(dy, B, H, W), slope))
        assert np.array_equal(bwd, orc.lrelu_bwd(fwd, dy, slope)) and np.array_equal(bwd, np.where(fwd > 0, dy, dy * np.float32(slope)))


@pytest.fixture(scope="module")
def adam_runs():
    """float64 runs of the Adam cases and torch's fp32 CPU runs of the same (the yardstick), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = ref.adam_case(name)
            p0, grads = ref.adam_inputs()
            run = ref.adam_reference_run(name)
            t32 = ref.adam_torch(p0, grads, ref.ADAM_LR, torch.float32, *ref.ADAM_BETAS, ref.ADAM_EPS, c["max_norm"], c["gscale"])
            yard = {}
            for step, (r, (p32, m32, v32)) in enumerate(zip(run, t32), 1):
                p_old = p0 if step == 1 else t32[step - 2][0].astype(np.float32)
                yard[step] = {k: close_ratio(a, b, fl, at) for k, (a, b, at, fl) in ref.adam_ratios(r, p_old, p32.astype(np.float32), m32, v32).items()}
            cache[name] = (c, run, yard)
        return cache[name]
    return get


def _adam_variant(F, variant, p, g, m, v, acc, c, step, state):
    b1, b2 = ref.ADAM_BETAS
    args = (acc, c["max_norm"], c["gscale"])
    if variant == "adam_step":
        F.adam_step(p, g, m, v, *args, ref.ADAM_LR, b1, b2, ref.ADAM_EPS, step)
    elif variant == "zero_grad":
        F.adam_step(p, g, m, v, *args, ref.ADAM_LR, b1, b2, ref.ADAM_EPS, step, zero_grad=True)
    elif variant == "bmax":
        F.adam_step_bmax(p, g, m, v, *args, ref.ADAM_LR, b1, b2, ref.ADAM_EPS, step, state["bmax"])
    else:
        F.adam_step_dev(p, g, m, v, *args, state["lr"], b1, b2, ref.ADAM_EPS, state["step"], state["scal"])


@pytest.mark.parametrize("variant", ["adam_step", "zero_grad", "dev", "bmax"])
@pytest.mark.parametrize("name", [c[0] for c in ref.ADAM_CASES])
def test_adam_vs_float64(F, adam_runs, name, variant):
    """clip + Adam over three steps, every entry point, against the float64 run of clip_grad_norm_ + torch.optim.Adam: m, v and the
    UPDATE p_new - p_old (not p, in whose magnitude a wrong update hides) through f64_gate at 1e-4 -- v and the update element-wise
    (floor 0), m relative to max(|m_old|, |g|) (the lerp can cancel), the update with half an ulp of p as its absolute floor.
    Gradients span 1e-9 .. 1e+1 with exact zeros (sqrt(v) / sqrt(bc2) crosses eps); cases: norm below max_norm, above it, no norm
    at all, gscale 1, 1/2, 1/3 (scale first, then clip the scaled norm).  tests/test_train_tail_ref.py shows the preconditions.
    All variants must produce the same bits; zero_grad leaves g zero; the device step counter counts 0 -> 3."""
    c, run, yard = adam_runs(name)
    p0, grads = ref.adam_inputs()
    n = ref.ADAM_N
    ch = F.adam_chunk()
    assert n > 2 * ch and (n % ch) % 256 != 0
    p, m, v = vec(p0.copy()), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pr, mr, vr = vec(p0.copy()), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = {"bmax": torch.empty(4 * ((n + ch - 1) // ch), device="cuda"), "lr": torch.tensor([ref.ADAM_LR], dtype=torch.float32, device="cuda"),
             "step": torch.zeros(1, dtype=torch.int64, device="cuda"), "scal": torch.empty(2, device="cuda")}
    for step, (r, g0) in enumerate(zip(run, grads), 1):
        g, acc = vec(g0.copy()), None
        if c["max_norm"] > 0:
            acc = F.sumsq_accumulator("cuda")
            F.sumsq(g, acc)
        p_old = p.cpu().numpy()
        _adam_variant(F, variant, p, g, m, v, acc, c, step, state)
        for what, (a, b, at, fl) in ref.adam_ratios(r, p_old, p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()).items():
            f64_gate(a, b, yard[step][what], f"{variant} {name} step {step} {what}", atol=at, floor=fl)
        assert np.array_equal(g.cpu().numpy(), np.zeros(n, np.float32) if variant == "zero_grad" else g0)
        if variant != "adam_step":                                  # the same bits as stem_adam_step with the same host values
            _adam_variant(F, "adam_step", pr, vec(g0.copy()), mr, vr, acc, c, step, state)
            assert torch.equal(p, pr) and torch.equal(m, mr) and torch.equal(v, vr)
        if variant == "dev":
            assert int(state["step"][0]) == step
        if variant == "bmax":
            pn = p.cpu().numpy()
            cmax = np.array([np.abs(pn[i:i + ch]).max() for i in range(0, n, ch)], np.float32)
            assert np.array_equal(state["bmax"].cpu().numpy().reshape(-1, 4).max(1), cmax)


def test_adam_step_dev_honours_a_rewritten_learning_rate(F):
    """the learning rate lives in device memory: rewritten between two steps (what a scheduler does between graph replays) it is the
    one the next step uses -- bit-equal to stem_adam_step given the new value on the host"""
    c = ref.adam_case("clip_gs_half")
    p0, grads = ref.adam_inputs()
    n = ref.ADAM_N
    p, m, v, pr, mr, vr = vec(p0.copy()), *(torch.zeros(n, device="cuda") for _ in range(2)), vec(p0.copy()), *(torch.zeros(n, device="cuda") for _ in range(2))
    lr_dev, step_dev, scal = torch.tensor([1e-3], device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), torch.empty(2, device="cuda")
    for step, (g0, lr) in enumerate(zip(grads, (1e-3, 2.5e-4, 7e-3)), 1):
        lr32 = float(np.float32(lr))
        lr_dev.fill_(lr32)
        g, acc = vec(g0), F.sumsq_accumulator("cuda")
        F.sumsq(g, acc)
        F.adam_step_dev(p, g, m, v, acc, c["max_norm"], c["gscale"], lr_dev, *ref.ADAM_BETAS, ref.ADAM_EPS, step_dev, scal)
        before = pr.clone()
        F.adam_step(pr, g, mr, vr, acc, c["max_norm"], c["gscale"], lr32, *ref.ADAM_BETAS, ref.ADAM_EPS, step)
        assert torch.equal(p, pr) and torch.equal(m, mr) and torch.equal(v, vr) and int(step_dev[0]) == step
        assert float((pr - before).abs().max()) > 0.5 * lr32                 # the update is as large as this step's rate
