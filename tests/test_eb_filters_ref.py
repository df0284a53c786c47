"""CPU: pins tests/eb_filters_ref.py, the float64 reference of the general EntropyBottleneck kernels --
  * against the reference's own module (tests/golden/eb_filters.npz, written by tests/golden/make_golden_eb_filters.py): likelihoods of
    both forwards, every parameter gradient and the input gradient, the auxiliary loss and its quantile gradient, per golden tuple;
  * against entropy_ref (the restatement through oracle/stem_torch_cpu.py, fixed at five layers) at (3, 3, 3, 3);
and shows the preconditions of its inputs: some elements are blocked in "mixed", none in "train", some likelihoods sit at the floor."""
import math
import os
import sys

import numpy as np
import pytest

import eb_filters_ref as ebr
import entropy_ref as er
import train_tail_ref as ref
from conftest import REPO, close_ratio

sys.path.insert(0, os.path.join(REPO, "oracle"))
# the references hand out read-only arrays (shared between tests); torch warns when it wraps one without copying
pytestmark = pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")

# float64 against float64 values that were stored rounded to float32 (2^-24 relative), after an fp32 rounding of dlik
TOL = 1e-6


def _pack_of(g, tag, filters):
    return np.concatenate([g[f"{tag}:sd:{name}"].reshape(g[f"{tag}:sd:{name}"].shape[0], -1) for name, _, _, _ in ebr.layout(filters)], axis=1)


def _flat(a):
    """[B, C, H, W] -> [npix, C]"""
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1))).reshape(-1, a.shape[1])


@pytest.mark.parametrize("filters", ebr.GOLDEN_TUPLES, ids=ebr.tuple_id)
def test_reference_restatement_matches_the_reference_module(golden, filters):
    g, tag = golden("eb_filters.npz"), ebr.tuple_id(filters)
    pack = _pack_of(g, tag, filters)
    assert pack.shape == (int(g["C"][0]), ebr.nparam(filters)) and pack.dtype == np.float32
    for mode in ("train", "eval"):
        lik = ebr.likelihood(_flat(g[f"{tag}:{mode}:z_hat"]), pack, filters)
        assert close_ratio(lik, _flat(g[f"{tag}:{mode}:lik"]), 0.1) < TOL, mode
    # the scalar of the generator: coef * sum(ln lik) + sum(w * z_hat) of the training forward
    x, z_hat = g[f"{tag}:x"], _flat(g[f"{tag}:train:z_hat"])
    coef = -1.0 / (math.log(2.0) * x.shape[0] * x.shape[2] * x.shape[3])
    dlik = (coef / ebr.likelihood(z_hat, pack, filters)).astype(np.float32)
    dz, dpack = ebr.backward(z_hat, pack, dlik, filters)
    assert close_ratio(dz + _flat(g[f"{tag}:w"]), _flat(g[f"{tag}:grad:x"]), 0.1) < TOL
    for name, got in ebr.pack_columns(dpack, filters):
        want = g[f"{tag}:grad:{name}"]
        assert close_ratio(got, want.reshape(want.shape[0], -1), 0.1) < TOL, name
    loss, dq = ebr.aux(g[f"{tag}:sd:quantiles"], pack, g[f"{tag}:sd:target"], filters)
    assert abs(loss - float(g[f"{tag}:aux"][0])) <= TOL * loss and close_ratio(dq, g[f"{tag}:aux:dq"], 0.1) < TOL
    assert np.array_equal(g[f"{tag}:sd:target"], ebr.AUX_TARGET)


def test_reference_restatement_matches_entropy_ref():
    """(3, 3, 3, 3): the packs, the inputs of both regimes and every float64 result are entropy_ref's, value for value"""
    f = (3, 3, 3, 3)
    assert [(n, s) for n, s, _, _ in ebr.layout(f)] == list(zip(er.EB_NAMES, er.EB_SHAPES))
    assert [o for _, _, o, _ in ebr.layout(f)] == er.EB_OFF and ebr.nparam(f) == er.NP
    assert np.array_equal(ebr.random_pack(5, f, 32), ref.eb_random_pack(5, 32))
    for shape in (ref.TAIL_SHAPES[0], ref.TAIL_SHAPES[3]):
        for regime in ebr.REGIMES:
            a, b = ebr.backward_case(shape, f, regime), er.eb_backward_case(shape, regime)
            assert all(np.array_equal(a[k], b[k]) for k in ("z_hat", "pack", "dlik", "blocked"))
            assert close_ratio(a["raw"], b["raw"], 0.0) < 1e-12
            ra, rb = ebr.backward_reference(shape, f, regime), er.eb_backward_reference(shape, regime)
            for k in ("dz", "dpack"):
                assert close_ratio(ra[k], rb[k], 0.1) < 1e-12, (regime, k)
                assert close_ratio(ra[k + "32"], rb[k + "32"], 0.1) < 1e-4, (regime, k)
    for C in (1, 86):
        (qa, pa, ta), (qb, pb, tb) = ebr.aux_inputs(C, f), er.aux_inputs(C)
        assert np.array_equal(qa, qb) and np.array_equal(pa, pb) and np.array_equal(ta, tb)
        ra, rb = ebr.aux_reference(C, f), er.aux_reference(C)
        assert abs(ra["loss"] - rb["loss"]) <= 1e-12 * rb["loss"] and close_ratio(ra["dq"], rb["dq"], 0.1) < 1e-12


@pytest.mark.parametrize("filters", ebr.TUPLES, ids=ebr.tuple_id)
def test_preconditions_of_the_inputs(filters):
    """4160 pixels x 5 channels: "train" blocks nothing (dlik < 0 everywhere), "mixed" blocks some elements and passes others whose
    raw likelihood is below the floor (dlik < 0 there); the float32 run of the reference stays inside the project's gate"""
    shape = ref.TAIL_SHAPES[3]
    tr, mx = ebr.backward_case(shape, filters, "train"), ebr.backward_case(shape, filters, "mixed")
    assert not tr["blocked"].any() and (tr["dlik"] < 0).all()
    below = mx["raw"] < ebr.LIK_BOUND
    assert mx["blocked"].any() and (below & ~mx["blocked"]).any() and (mx["raw"] < 0.5e-9).mean() > 0.01
    assert tr["pack"].shape == (5, ebr.nparam(filters))
    r = ebr.backward_reference(shape, filters, "mixed")
    assert (r["dz"][mx["blocked"]] == 0).all() and (r["dz"][~mx["blocked"]] != 0).any()
    worst = max([close_ratio(r["dz32"], r["dz"], 0.1)] + [close_ratio(a, b, 0.1) for (_, a), (_, b) in
                                                          zip(ebr.pack_columns(r["dpack32"], filters), ebr.pack_columns(r["dpack"], filters))])
    print(f"{ebr.tuple_id(filters)}: the reference's float32 run is at most {worst:.2e} from float64")
    assert worst < 1e-4
    assert ebr.gate_rtol(2e-5) == (1e-4, False) and ebr.gate_rtol(5e-5) == (3.0 * 5e-5, True) and ebr.gate_rtol(3.4e-5)[0] > 1e-4
