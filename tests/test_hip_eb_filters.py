"""GPU parity tests, op level, for the EntropyBottleneck kernels of any `filters` tuple (csrc/eb_filters.hip, include/stem_eb_filters.h):
forward (both modes), backward, auxiliary loss, pack / unpack, each called on its own and compared with tests/eb_filters_ref.py (pinned
on the CPU by tests/test_eb_filters_ref.py) -- bit for bit where the operation is exact (one fp32 add, rounding, copies, blocked
gradients), through conftest.f64_gate against float64 where it is fp32 arithmetic.

Shapes: train_tail_ref.TAIL_SHAPES -- 198 pixels (less than one pass of a workgroup), 4096, 4160 (sixteen passes and a partial one),
C = 3 and 5 -- and one case of 320 channels.  Tuples: eb_filters_ref.TUPLES -- () (one layer, no gate, 2 floats), (1,), (5,),
(3, 3, 3), (3, 3, 3, 3) (beside the specialised kernels), (2, 4, 8) (in != out in every matrix), (8,) * 6 (both caps at once).

The gate is conftest.f64_gate's 1e-4 (floor 0.1).  Where the float32 run of the reference is itself more than 3.3e-5 from float64 on a
tensor, that tensor's bound is max(1e-4, 3 x that distance) (tests/test_hip_spread.py's rule, eb_filters_ref.gate_rtol); the distance
is printed and the tensors concerned are named."""
import numpy as np
import pytest
import torch

import eb_filters_ref as ebr
import entropy_ref as er
import train_tail_ref as ref
from conftest import close_ratio, f64_gate
from test_hip_train_tail import flat, nhwc, vec

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

BOUND32 = float(np.float32(1e-9))
WIDE_SHAPE = (1, 6, 11, 320)          # 320 workgroups in the backward: more than one round of the eight XCDs' 32 compute units


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return functional


def _id(s):
    return "B%d_%dx%d_C%d" % s


def gate(ours, exact, y32, what, **kw):
    """f64_gate at eb_filters_ref.gate_rtol(the reference's own float32 distance); -> True where the wider bound applied"""
    rtol, widened = ebr.gate_rtol(y32)
    if widened:
        print(f"[wider gate] {what}: the reference's float32 run is {y32:.2e} from float64 -> bound {rtol:.2e}")
    f64_gate(ours, exact, y32, what, rtol=rtol, **kw)
    return widened


# =========================================================================================================== forward
@pytest.mark.parametrize("filters", ebr.TUPLES, ids=ebr.tuple_id)
@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_id)
def test_forward_vs_float64(F, shape, filters):
    """stem_ebf_forward, z a channel slice of a wider buffer of NaNs (ldz = C + 3): noise mode gives z + noise exactly, eval mode
    rintf(z - median) + median exactly; the likelihoods of both against float64; elements whose raw likelihood is below the floor
    hold the floor exactly"""
    B, H, W, C = shape
    c = ebr.forward_case(shape, filters)
    zd, pd = nhwc(c["z"], B, H, W, ld=C + 3, c0=1), vec(c["pack"])
    assert F.nhwc_ld(zd) == C + 3
    m = c["medians"]
    cases = (("noise", {"noise": nhwc(c["noise"], B, H, W)}, c["z"] + c["noise"]), ("eval", {"medians": vec(m)}, np.rint(c["z"] - m) + m))
    for mode, kw, want in cases:
        z_hat, lik = F.ebf_forward(zd, pd, filters, **kw)
        assert F.nhwc_ld(z_hat) == C and F.nhwc_ld(lik) == C
        zh = flat(z_hat)
        assert np.array_equal(zh, want.astype(np.float32)), mode
        raw = ebr.raw_likelihood(zh, c["pack"], filters)
        exact = np.maximum(raw, 1e-9)
        y32 = close_ratio(ebr.likelihood(zh, c["pack"], filters, torch.float32), exact, 0.1, 1e-9)
        gate(flat(lik), exact, y32, f"ebf_forward {ebr.tuple_id(filters)} {mode} lik {_id(shape)}", atol=1e-9)
        floor = raw < 0.5e-9
        assert floor.any() and np.array_equal(flat(lik)[floor], np.full(int(floor.sum()), BOUND32, np.float32)), mode


# =========================================================================================================== backward
@pytest.mark.parametrize("regime", ebr.REGIMES)
@pytest.mark.parametrize("filters", ebr.TUPLES, ids=ebr.tuple_id)
@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_id)
def test_backward_vs_float64(F, shape, filters, regime):
    """stem_ebf_backward against float64 autograd: dz and every column group of dpack through the gate.  Exact: blocked elements
    (raw likelihood below 1e-9 and dlik >= 0) give zeros, or dzhat_in where given; dzhat_in is one fp32 add; either output may be
    left out; two launches agree bit for bit; the outputs, allocated NaN-filled between NaN sentinels, come back fully written with the
    sentinels intact."""
    B, H, W, C = shape
    n, NP = B * H * W, ebr.nparam(filters)
    c, r = ebr.backward_case(shape, filters, regime), ebr.backward_reference(shape, filters, regime)
    what = f"ebf_backward {ebr.tuple_id(filters)} {regime} {_id(shape)}"
    zh, pd, dl = nhwc(c["z_hat"], B, H, W), vec(c["pack"]), nhwc(c["dlik"], B, H, W)
    G = 64
    dz_buf = torch.full((n * C + 2 * G,), float("nan"), device="cuda")
    dp_buf = torch.full((C * NP + 2 * G,), float("nan"), device="cuda")
    dz_t, dpack_t = F.ebf_backward(zh, pd, dl, filters, dz_out=dz_buf[G:G + n * C].view(B, H, W, C).permute(0, 3, 1, 2),
                                   dpack_out=dp_buf[G:G + C * NP].view(C, NP))
    for buf, m in ((dz_buf, n * C), (dp_buf, C * NP)):
        assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + m:]).all() and not torch.isnan(buf[G:G + m]).any()
    dz, dpack = flat(dz_t), dpack_t.cpu().numpy()
    wide = []
    if gate(dz, r["dz"], close_ratio(r["dz32"], r["dz"], 0.1), what + " dz"):
        wide.append("dz")
    for (name, got), (_, exact), (_, y32) in zip(ebr.pack_columns(dpack, filters), ebr.pack_columns(r["dpack"], filters),
                                                 ebr.pack_columns(r["dpack32"], filters)):
        if gate(got, exact, close_ratio(y32, exact, 0.1), f"{what} dpack{name}"):
            wide.append(name)
    print(f"[{what}] tensors under the wider gate: {wide or 'none'}")
    blocked = c["blocked"]
    assert blocked.any() == (regime == "mixed")
    assert np.array_equal(dz[blocked], np.zeros(int(blocked.sum()), np.float32)) and np.array_equal(dz != 0, r["dz"] != 0)
    # dzhat_in: one fp32 add per element
    dzin = np.random.default_rng(6).uniform(-1.0, 1.0, dz.shape).astype(np.float32) * np.float32(np.abs(dz).max())
    dz_w, dpack_w = F.ebf_backward(zh, pd, dl, filters, dzhat_in=nhwc(dzin, B, H, W))
    assert np.array_equal(flat(dz_w), dz + dzin) and torch.equal(dpack_w, dpack_t)
    assert np.array_equal(flat(dz_w)[blocked], dzin[blocked])
    # a second launch: the same bits.  Either output left out: the other one is unchanged (dz alone comes from a kernel instance of its
    # own: held to float64 and to the exact zeros)
    dz_2, dpack_2 = F.ebf_backward(zh, pd, dl, filters)
    assert torch.equal(dz_2, dz_t) and torch.equal(dpack_2, dpack_t)
    none, dpack_only = F.ebf_backward(zh, pd, dl, filters, want_dz=False)
    assert none is None and torch.equal(dpack_only, dpack_t)
    dz_only, none = F.ebf_backward(zh, pd, dl, filters, want_dpack=False)
    assert none is None
    gate(flat(dz_only), r["dz"], close_ratio(r["dz32"], r["dz"], 0.1), what + " dz alone")
    assert np.array_equal(flat(dz_only)[blocked], np.zeros(int(blocked.sum()), np.float32))
    print(f"[{what}] max |dz alone - dz| = {np.abs(flat(dz_only) - dz).max():.3e}")


@pytest.mark.parametrize("filters", [(3, 3, 3), (8,) * 6], ids=ebr.tuple_id)
def test_backward_channels_do_not_leak(F, filters):
    """row c of dpack and column c of dz from a C-channel call == those of a one-channel call on channel c alone, bit for bit (c = 0
    and C - 1; 4160 pixels): nothing crosses between workgroups, and the channel stride of the loads is right"""
    shape = ref.TAIL_SHAPES[3]
    B, H, W, C = shape
    c = ebr.backward_case(shape, filters, "mixed")
    dz_t, dpack_t = F.ebf_backward(nhwc(c["z_hat"], B, H, W), vec(c["pack"]), nhwc(c["dlik"], B, H, W), filters)
    for ch in (0, C - 1):
        one = slice(ch, ch + 1)
        dz1, dpack1 = F.ebf_backward(nhwc(c["z_hat"][:, one], B, H, W), vec(c["pack"][one]), nhwc(c["dlik"][:, one], B, H, W), filters)
        assert torch.equal(dpack1[0], dpack_t[ch]) and np.array_equal(flat(dz1)[:, 0], flat(dz_t)[:, ch])


def test_320_channels(F):
    """(2, 4, 8) on 66 pixels x 320 channels: twenty channel tiles of the forward, 320 workgroups of the backward"""
    filters, shape = (2, 4, 8), WIDE_SHAPE
    B, H, W, C = shape
    c, r = ebr.backward_case(shape, filters, "mixed"), ebr.backward_reference(shape, filters, "mixed")
    f = ebr.forward_case(shape, filters)
    z_hat, lik = F.ebf_forward(nhwc(f["z"], B, H, W), vec(f["pack"]), filters, noise=nhwc(f["noise"], B, H, W))
    assert np.array_equal(flat(z_hat), c["z_hat"])
    exact = np.maximum(c["raw"], 1e-9)
    gate(flat(lik), exact, close_ratio(ebr.likelihood(c["z_hat"], c["pack"], filters, torch.float32), exact, 0.1, 1e-9),
         "ebf_forward C=320 lik", atol=1e-9)
    dz_t, dpack_t = F.ebf_backward(z_hat, vec(c["pack"]), nhwc(c["dlik"], B, H, W), filters)
    gate(flat(dz_t), r["dz"], close_ratio(r["dz32"], r["dz"], 0.1), "ebf_backward C=320 dz")
    dpack = dpack_t.cpu().numpy()
    for (name, got), (_, want), (_, y32) in zip(ebr.pack_columns(dpack, filters), ebr.pack_columns(r["dpack"], filters),
                                                ebr.pack_columns(r["dpack32"], filters)):
        gate(got, want, close_ratio(y32, want, 0.1), f"ebf_backward C=320 dpack{name}")


# =========================================================================================================== auxiliary loss
@pytest.mark.parametrize("filters", [(3, 3, 3), (8,) * 6], ids=ebr.tuple_id)
@pytest.mark.parametrize("C", er.AUX_CHANNELS)
def test_aux_loss_vs_float64(F, C, filters):
    """stem_ebf_aux_loss_grad (one workgroup, channels in chunks of 32: its LDS does not depend on C) against float64 from 1 to 688
    channels: the loss at 1e-4 relative, dq element-wise; accumulate=True adds in one fp32 add; loss_out is the tensor handed in and is
    written, not added to; two launches agree bit for bit"""
    q, pack, target = ebr.aux_inputs(C, filters)
    r = ebr.aux_reference(C, filters)
    what = f"ebf_aux_loss_grad {ebr.tuple_id(filters)} C={C}"
    qd, pd, td = vec(q), vec(pack), vec(target)
    dq_t = torch.full((C, 1, 3), float("nan"), device="cuda")
    loss_in = torch.full((1,), float("nan"), device="cuda")
    loss_t = F.ebf_aux_loss_grad(qd, pd, td, filters, dq_t, loss_out=loss_in)
    assert loss_t is loss_in
    dq = dq_t.cpu().numpy()
    gate(float(loss_t[0]), r["loss"], abs(r["loss32"] - r["loss"]) / r["loss"], what + " loss", floor=0.0)
    gate(dq, r["dq"], close_ratio(r["dq32"], r["dq"], 0.1), what + " dq")
    dq0 = np.random.default_rng(8).uniform(-30.0, 30.0, (C, 1, 3)).astype(np.float32)
    acc = vec(dq0.copy())
    loss_a = F.ebf_aux_loss_grad(qd, pd, td, filters, acc, accumulate=True)
    assert np.array_equal(acc.cpu().numpy(), dq0 + dq) and torch.equal(loss_a, loss_t)
    loss_n = F.ebf_aux_loss_grad(qd, pd, td, filters, None, loss_out=torch.full((1,), 7.0, device="cuda"))
    assert torch.equal(loss_n, loss_t)


# =========================================================================================================== pack / unpack
@pytest.mark.parametrize("filters", ebr.TUPLES, ids=ebr.tuple_id)
def test_pack_and_unpack_are_copies(F, filters):
    """stem_ebf_pack / stem_ebf_unpack_grads against numpy, bit for bit (C = 5 and 300: one and several workgroups); accumulate is one
    fp32 add; at (3, 3, 3, 3) the image is F.eb_pack's"""
    for C in (5, 300):
        pack = ebr.random_pack(C, filters, 90 + C)
        lay = ebr.layout(filters)
        tensors = [vec(pack[:, o:o + n].reshape(C, *shape)) for _, shape, o, n in lay]
        got = F.ebf_pack(tensors, filters)
        assert tuple(got.shape) == (C, ebr.nparam(filters)) and np.array_equal(got.cpu().numpy(), pack)
        if filters == (3, 3, 3, 3):
            assert torch.equal(got, F.eb_pack(tensors))
        grads = [torch.full((C, *shape), float("nan"), device="cuda") for _, shape, _, _ in lay]
        F.ebf_unpack_grads(got, grads, filters)
        for g, (_, shape, o, n) in zip(grads, lay):
            assert np.array_equal(g.cpu().numpy(), pack[:, o:o + n].reshape(C, *shape))
        base = [np.random.default_rng(91 + i).uniform(-1, 1, (C, *shape)).astype(np.float32) for i, (_, shape, _, _) in enumerate(lay)]
        acc = [vec(b.copy()) for b in base]
        F.ebf_unpack_grads(got, acc, filters, accumulate=True)
        for a, b, (_, shape, o, n) in zip(acc, base, lay):
            assert np.array_equal(a.cpu().numpy(), b + pack[:, o:o + n].reshape(C, *shape))


# =========================================================================================================== general against specialised
@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_id)
def test_general_beside_specialised(F, shape):
    """(3, 3, 3, 3): the general and the specialised kernels on the same inputs, both through the gate against the same float64
    values.  Their largest mutual difference is printed, not asserted: the two bodies may be contracted differently."""
    filters = (3, 3, 3, 3)
    B, H, W, C = shape
    c, r = ebr.backward_case(shape, filters, "mixed"), ebr.backward_reference(shape, filters, "mixed")
    f = ebr.forward_case(shape, filters)
    zd, nd, pd = nhwc(f["z"], B, H, W), nhwc(f["noise"], B, H, W), vec(f["pack"])
    exact = np.maximum(c["raw"], 1e-9)
    y32 = close_ratio(ebr.likelihood(c["z_hat"], c["pack"], filters, torch.float32), exact, 0.1, 1e-9)
    (zg, lg), (zs, ls) = F.ebf_forward(zd, pd, filters, noise=nd), F.eb_forward(zd, pd, noise=nd)
    assert torch.equal(zg, zs)
    for name, lik in (("general", lg), ("specialised", ls)):
        gate(flat(lik), exact, y32, f"{name} forward lik {_id(shape)}", atol=1e-9)
    dl = nhwc(c["dlik"], B, H, W)
    (dzg, dpg), (dzs, dps) = F.ebf_backward(zg, pd, dl, filters), F.eb_backward(zs, pd, dl)
    for name, dz, dp in (("general", dzg, dpg), ("specialised", dzs, dps)):
        gate(flat(dz), r["dz"], close_ratio(r["dz32"], r["dz"], 0.1), f"{name} backward dz {_id(shape)}")
        for (col, got), (_, want), (_, w32) in zip(ebr.pack_columns(dp.cpu().numpy(), filters), ebr.pack_columns(r["dpack"], filters),
                                                   ebr.pack_columns(r["dpack32"], filters)):
            gate(got, want, close_ratio(w32, want, 0.1), f"{name} backward dpack{col} {_id(shape)}")
    q, pack, target = ebr.aux_inputs(C, filters)
    a = ebr.aux_reference(C, filters)
    dqg, dqs = torch.empty((C, 1, 3), device="cuda"), torch.empty((C, 1, 3), device="cuda")
    lg_ = F.ebf_aux_loss_grad(vec(q), vec(pack), vec(target), filters, dqg)
    ls_ = F.eb_aux_loss_grad(vec(q), vec(pack), vec(target), dqs)
    for name, loss, dq in (("general", lg_, dqg), ("specialised", ls_, dqs)):
        gate(float(loss[0]), a["loss"], abs(a["loss32"] - a["loss"]) / a["loss"], f"{name} aux loss C={C}", floor=0.0)
        gate(dq.cpu().numpy(), a["dq"], close_ratio(a["dq32"], a["dq"], 0.1), f"{name} aux dq C={C}")
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    print(f"[general - specialised, {_id(shape)}] relative to the tensor's maximum: lik {rel(lg, ls):.2e}  dz {rel(dzg, dzs):.2e}  "
          f"dpack {rel(dpg, dps):.2e}  dq {rel(dqg, dqs):.2e}  loss {abs(float(lg_[0]) - float(ls_[0])) / float(ls_[0]):.2e}")
