"""CPU suite for tests/entropy_ref.py: the references that tests/test_hip_entropy_ops.py holds the entropy-model kernels to are pinned
here (the C oracle on the golden case, hand-checkable points, two independent statements of the same thing), and every precondition
its gates and exact assertions rest on is shown on the inputs alone, so that no GPU test can pass vacuously.  The argument checks of
stem_eb_aux_loss_grad run before anything touches a device and are tested here too."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import entropy_ref as er
import train_tail_ref as ref
from conftest import REPO, assert_close, close_ratio

sys.path.insert(0, os.path.join(REPO, "oracle"))
import stem_oracle as orc  # noqa: E402


def _id(s):
    return "B%d_%dx%d_C%d" % s


# ---------------------------------------------------------------------------------------------------------------- EntropyBottleneck backward
def test_pack_columns_are_the_oracles():
    """EB_OFF / EB_LEN (kOff / kLen of csrc/entropy.hip) cut a [C,58] pack where orc.eb_unpack_grads cuts it"""
    assert er.EB_OFF == [0, 3, 6, 9, 18, 21, 24, 33, 36, 39, 48, 51, 54, 57] and er.EB_LEN == [3, 3, 3, 9, 3, 3, 9, 3, 3, 9, 3, 3, 3, 1]
    dpack = np.arange(5 * 58, dtype=np.float32).reshape(5, 58)
    un = orc.eb_unpack_grads(dpack)
    for name, cols in er.pack_columns(dpack):
        assert np.array_equal(un["entropy_bottleneck." + name].reshape(5, -1), cols)
    sd = {k: t.numpy() for k, t in ref.eb_state_dict(dpack, torch.float32).items()}
    assert np.array_equal(orc.eb_pack_params(sd), dpack)


def test_eb_backward_reference_vs_c_oracle(golden):
    """the float64 autograd reference against orc.eb_likelihood_bwd (the C oracle, itself pinned to the reference project's gradients
    by test_oracle_vs_golden.py) on the golden case: dz and every parameter tensor of dpack"""
    from spatiotemporalentropymodel_amd.weights import closed_form_input
    g = golden("ops_small.npz")
    sd = {k[len("eb:p:"):]: v for k, v in g.items() if k.startswith("eb:p:")}
    pack = orc.eb_pack_params(sd, prefix="")
    x = g["eb:x"]
    v = orc.nchw_to_cl(x) + closed_form_input("noise:eb:0", (4, 1, 2 * 3 * 5), -0.5, 0.5).numpy().reshape(4, -1)
    dlik = orc.nchw_to_cl(g["eb:dlik"])
    dv, dp = orc.eb_likelihood_bwd(v, pack, dlik)
    dz, dpack, A = er.eb_backward(v.T, pack, dlik.T)
    assert_close(dv.T, dz, what="dz", floor=0.1)
    for (name, a), (_, b) in zip(er.pack_columns(dp), er.pack_columns(dpack)):
        assert_close(a, b, what="dpack " + name, floor=0.1)
    for name, gr in orc.eb_unpack_grads(dpack.astype(np.float32), prefix="").items():
        assert_close(gr, g[f"eb:g:{name}"], what="golden " + name, floor=0.1)
    assert (A >= np.abs(dpack) * (1 - 1e-12)).all()


def test_eb_backward_reference_by_hand():
    """one sample whose likelihood is far above the floor: dz against a central difference of the float64 likelihood, and a blocked
    sample (raw likelihood below 1e-9, positive dlik) with gradient exactly zero while the same sample with a negative dlik passes"""
    pack = ref.eb_random_pack(2, 7)
    z = np.array([[0.3, -1.2], [40.0, 40.0]], np.float32)
    dlik = np.array([[1.5, -0.75], [2.0, -2.0]], np.float32)
    dz, dpack, A = er.eb_backward(z, pack, dlik)
    h = 2.0 ** -10                                                      # exact steps in fp32 at |z| ~ 1
    num = (er.eb_raw_likelihood(z + np.float32(h), pack) - er.eb_raw_likelihood(z - np.float32(h), pack)) / (2 * h)
    assert np.abs(dz[0] - num[0] * dlik[0]).max() < 1e-5 * np.abs(dz[0]).max()
    assert (er.eb_raw_likelihood(z, pack)[1] < 1e-9).all()
    assert dz[1, 0] == 0.0 and dz[1, 1] != 0.0
    only_first = er.eb_backward(z[:1], pack, dlik[:1])[1]
    assert np.array_equal(dpack[0], only_first[0]) and not np.array_equal(dpack[1], only_first[1])


@pytest.mark.parametrize("shape", [ref.TAIL_SHAPES[0], ref.TAIL_SHAPES[3]], ids=_id)
def test_eb_backward_preconditions(shape):
    """What test_eb_backward_vs_float64 assumes, on the inputs and the reference alone (the smallest and the largest shape):
      - at least 4 % of the likelihoods are at the floor, and none is within 1e-3 of it (the LowerBound mask is the same in fp32);
      - train: every dlik is negative, nothing is blocked, |dpack| >= 1e-3 A for at least 90 % of the (c, k) entries;
      - mixed: at least 1.5 % of the elements are blocked, at least as many floor elements pass, blocked dz is exactly zero;
      - the float32 run of the reference is within 1e-4 / 4 of the float64 run in every gated quantity;
      - A is the sum of the two branches' magnitudes: A >= |dpack|."""
    for regime in er.EB_REGIMES:
        c, r = er.eb_backward_case(shape, regime), er.eb_backward_reference(shape, regime)
        raw, dlik = c["raw"], c["dlik"]
        floor = raw < 1e-9
        assert floor.mean() >= 0.04 and np.abs(raw / 1e-9 - 1.0).min() > 1e-3
        if regime == "train":
            assert (dlik < 0).all() and not c["blocked"].any()
            assert (np.abs(r["dpack"]) >= 1e-3 * r["A"]).mean() >= 0.9
        else:
            assert c["blocked"].mean() >= 0.015 and (floor & (dlik < 0)).sum() >= c["blocked"].sum()
            assert (r["dz"][c["blocked"]] == 0).all() and (r["dz"][~c["blocked"]] != 0).all()
        assert (r["A"] >= np.abs(r["dpack"]) * (1 - 1e-12)).all() and (r["A"] > 0).all()
        assert close_ratio(r["dz32"], r["dz"], 0.1) <= 1e-4 / 4
        for (name, a), (_, b) in zip(er.pack_columns(r["dpack32"]), er.pack_columns(r["dpack"])):
            assert close_ratio(a, b, 0.1) <= 1e-4 / 4, name
        assert (np.abs(r["dpack32"] - r["dpack"]) / r["A"]).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- auxiliary loss
def test_aux_reference_vs_c_oracle_and_inputs():
    """eb_aux in float64 against orc.eb_aux_loss; no logit sits near its target (|d| > 1e-3: the sign, i.e. dq, is the same in fp32);
    the channel counts are the ones that matter to the two kernels"""
    assert er.AUX_CHANNELS == (1, 85, 86, 256, 257, 320, 688)
    assert 85 * 3 < 256 < 86 * 3 and 256 * 3 == 768 and er.AUX_MAX_C * 58 * 4 + (256 + 768) * 4 <= 160 * 1024 < (er.AUX_MAX_C + 1) * 58 * 4 + (256 + 768) * 4
    t = math.log(2.0 / 1e-9 - 1.0)
    assert np.array_equal(er.AUX_TARGET, np.array([-t, 0.0, t], np.float32))
    for C in er.AUX_CHANNELS:
        q, pack, target = er.aux_inputs(C)
        r = er.aux_reference(C)
        assert q.shape == (C, 1, 3) and np.abs(q).max() < 8.0 and np.abs(r["d"]).min() > 1e-3
        loss, dq = orc.eb_aux_loss(q, pack, target)
        assert abs(loss - r["loss"]) <= 1e-5 * r["loss"] and abs(r["loss"] - np.abs(r["d"]).sum()) <= 1e-12 * r["loss"]
        assert_close(dq, r["dq"], what=f"aux dq C={C}", floor=0.1)
        assert abs(r["loss32"] - r["loss"]) <= 1e-4 / 4 * r["loss"] and close_ratio(r["dq32"], r["dq"], 0.1) <= 1e-4 / 4


def _hip():
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


def test_eb_aux_loss_grad_argument_errors():
    """C = 689 (one channel more than one workgroup's LDS holds), C = 0 and a null quantiles / pack / target / loss pointer are refused
    before anything is launched; the message names the function.  The pointers are never dereferenced."""
    h = _hip()
    p = 4096
    ok = dict(quantiles=p, pack=p, target3=p, loss=p, dq=p, C=256)

    def call(**kw):
        a = dict(ok, **kw)
        rc = h.stem_eb_aux_loss_grad(a["quantiles"], a["pack"], a["target3"], a["loss"], a["dq"], a["C"], 0, None)
        return rc, h.stem_last_error()

    for bad in (dict(C=er.AUX_MAX_C + 1), dict(C=0), dict(C=-1), dict(quantiles=None), dict(pack=None), dict(target3=None), dict(loss=None)):
        rc, msg = call(**bad)
        assert rc != 0 and b"stem_eb_aux_loss_grad" in msg, (bad, rc, msg)
    assert b"689" in call(C=er.AUX_MAX_C + 1)[1]


# ---------------------------------------------------------------------------------------------------------------- eval-mode inputs
@pytest.mark.parametrize("shape", ref.TAIL_SHAPES, ids=_id)
def test_eval_inputs_hold_exact_ties(shape):
    """every channel of the EntropyBottleneck input has z - median == k + 1/2 exactly for an even and an odd k, rounded to the even
    neighbour by the reference expression; every 13th GaussianConditional element likewise; the rounded latents reach the floor"""
    B, H, W, C = shape
    z, med = er.eb_eval_inputs(B, H, W, C, 33)
    d = z[:4] - med
    assert np.array_equal(d, np.repeat(np.array([-2.5, 2.5, 0.5, -0.5], np.float32)[:, None], C, axis=1))
    zq = er.round_about(z, med)
    assert np.array_equal(zq[:4] - med, np.repeat(np.array([-2.0, 2.0, 0.0, -0.0], np.float32)[:, None], C, axis=1))
    assert np.array_equal(zq, orc.quantize_dequantize(z.T.copy(), med[:, None]).T)
    assert (ref.eb_likelihood(zq, ref.eb_random_pack(C, 32)) == 1e-9).mean() >= 0.02
    y, sc, mu = er.gc_eval_inputs(B, H, W, C, 43)
    t = er.gc_tie_mask(B * H * W, C)
    frac = (y - mu)[t] - np.floor((y - mu)[t])
    assert (frac == 0.5).all() and {int(k) for k in np.floor((y - mu)[t])} == set(er.GC_TIE_K)
    out = er.round_about(y, mu)
    assert np.array_equal(out, orc.quantize_dequantize(y, mu)) and ((out - mu)[t] % 2 == 0).all()
    # every 16th element is 7 .. 9 from its mean at a scale <= 1: 6.5 or more after rounding, below the floor for all but the widest
    assert (ref.gc_likelihood(out, sc, mu) == 1e-9).mean() >= 0.04 and (sc < 0.11).mean() > 0.2


# ---------------------------------------------------------------------------------------------------------------- table indexes
def test_index_references_agree_at_the_table_entries(golden):
    """orc.build_indexes == the searchsorted statement on scales that sit at, just below and just above every entry of the golden
    scale table; an entry itself belongs to its own index (s <= table[t]), its upper neighbour to the next; every index occurs"""
    table = golden("codec.npz")["gc:scale_table"]
    T = len(table)
    assert T == 64 and table[0] == np.float32(0.11) and (np.diff(table) > 0).all()
    s = er.index_scales(table)
    B, H, W, C = er.INDEX_SHAPE
    assert s.shape == (B * H * W, C) and s.size % 256 != 0 and s.size > 512
    idx = er.build_indexes(s, table)
    assert np.array_equal(idx, orc.build_indexes(s, table))
    assert set(idx.ravel().tolist()) == set(range(T))
    up = np.nextafter(table, np.float32(np.inf))
    assert np.array_equal(er.build_indexes(table, table), np.arange(T))
    assert np.array_equal(er.build_indexes(up, table), np.minimum(np.arange(T) + 1, T - 1))
    assert np.array_equal(er.build_indexes(np.nextafter(table, np.float32(-np.inf)), table), np.arange(T))
    assert np.array_equal(er.build_indexes(np.array([0.0, -1.0, 1e9], np.float32), table), [0, 0, T - 1])
    for v in np.concatenate([table, up, [np.float32(0.0)]]):
        assert (s == v).any()


def test_log2_likelihoods_span_the_range():
    lik = er.log2_likelihoods()
    assert lik.size == er.LOG2_SIZES[-1] > 1024 * 256 and lik.min() == np.float32(1e-9) and lik.max() <= 1.0
    assert er.LOG2_SIZES[1] == 1024 * 256 and np.log2(lik.astype(np.float64)).min() < -29.8
