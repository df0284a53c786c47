"""CPU: the host-side keys that decide whether a packed weight copy or a host CDF table is still current -- layers._PackCache,
StemEngine._weights_key, EntropyModel.host_tables -- under every way a parameter can change (tests/cache_cases.py).  No kernel
runs here: the builders are counters.  tests/test_hip_weight_caches.py checks the same contract through the kernels."""
import pytest
import torch

import cache_cases as cc
from spatiotemporalentropymodel_amd import layers
from spatiotemporalentropymodel_amd.layers import Conv2d, FusedSequential, GDN, bump_weight_epoch

ROLE, OTHER_ROLE = layers.PACK_F16X2, layers.PACK_F16X2_GEN


class Build:
    """a counting `build`: every call returns a new object"""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def _conv():
    return cc.make(Conv2d, 4, 4, 3, padding=1)


def _pair():
    """a convolution and a GDN: the two parameters of one PACK_C4GDN entry"""
    return cc.make(FusedSequential, cc.make(Conv2d, 3, 4, 3, padding=1), cc.make(GDN, 4))


def test_one_build_then_hits():
    m, build = _conv(), Build()
    first = m._packs._cached(ROLE, (m.weight,), build)
    for _ in range(3):
        assert m._packs._cached(ROLE, (m.weight,), build) is first
    assert build.calls == 1


@pytest.mark.parametrize("name", list(cc.CPU_MUTATIONS))
def test_each_visible_mutation_rebuilds_exactly_once(name):
    mutate = cc.CPU_MUTATIONS[name]
    m, build = _conv(), Build()
    cc.prepare(mutate, m)
    get = lambda: m._packs._cached(ROLE, cc.lookup(m, ["weight"]), build)
    first = get()
    assert get() is first and build.calls == 1
    before = m.weight.detach().clone()
    mutate(m, cc.lookup(m, ["weight"]))
    assert not torch.equal(m.weight.detach(), before), "the mutation did not move the weight"
    second = get()
    assert second is not first and build.calls == 2, f"{name}: the key missed the change"
    assert get() is second and build.calls == 2


@pytest.mark.parametrize("which", ["0.weight", "1.gamma"])
@pytest.mark.parametrize("name", list(cc.CPU_MUTATIONS))
def test_two_tensor_entry_rebuilds_when_either_tensor_changes(name, which):
    """the shape of call of get_c4gdn: one entry keyed on (weight, gamma)"""
    mutate = cc.CPU_MUTATIONS[name]
    m, build = _pair(), Build()
    cc.prepare(mutate, m)
    cache = m[0]._packs
    get = lambda: cache._cached(layers.PACK_C4GDN, cc.lookup(m, ["0.weight", "1.gamma"]), build)
    first = get()
    assert get() is first and build.calls == 1
    mutate(m, cc.lookup(m, [which]))
    assert get() is not first and build.calls == 2, f"{name} of {which} alone: the key missed the change"
    get()
    assert build.calls == 2


def test_roles_do_not_evict_each_other():
    m, a, b = _conv(), Build(), Build()
    pa = m._packs._cached(ROLE, (m.weight,), a)
    pb = m._packs._cached(OTHER_ROLE, (m.weight,), b)
    assert pa is not pb
    assert m._packs._cached(ROLE, (m.weight,), a) is pa and m._packs._cached(OTHER_ROLE, (m.weight,), b) is pb
    assert (a.calls, b.calls) == (1, 1)
    cc.inplace_no_grad(m, [m.weight])                     # ... and a change reaches both
    assert m._packs._cached(ROLE, (m.weight,), a) is not pa and m._packs._cached(OTHER_ROLE, (m.weight,), b) is not pb
    assert (a.calls, b.calls) == (2, 2)


def test_data_write_is_invisible_until_the_epoch_is_bumped():
    """INTEGRATION.md, "Writing weights through .data": an in-place write through `.data` moves neither the version counter nor the
    address, so the cache keeps the old copy (pinned here as the documented behaviour); bump_weight_epoch(params) marks those
    tensors alone, bump_weight_epoch() everything."""
    m, other = _conv(), _conv()
    bm, bo = Build(), Build()
    gm = lambda: m._packs._cached(ROLE, (m.weight,), bm)
    go = lambda: other._packs._cached(ROLE, (other.weight,), bo)
    pm, po = gm(), go()
    before = m.weight.detach().clone()
    cc.STALE_MUTATION(m, [m.weight])
    assert torch.equal(m.weight.detach(), before * cc.FACTOR)
    assert gm() is pm and bm.calls == 1                   # stale, as documented
    bump_weight_epoch([m.weight])
    pm2 = gm()
    assert pm2 is not pm and bm.calls == 2
    assert go() is po and bo.calls == 1                   # the per-parameter form leaves another parameter's entry valid
    assert gm() is pm2 and bm.calls == 2
    bump_weight_epoch()                                   # the global form invalidates all
    assert gm() is not pm2 and go() is not po
    assert (bm.calls, bo.calls) == (3, 2)
    gm(), go()
    assert (bm.calls, bo.calls) == (3, 2)


def test_a_build_that_writes_the_tensor_does_not_cause_a_rebuild():
    """what the masked pack does: it zeroes taps of `weight` in place while packing, so the key is taken after the build"""
    m = _conv()
    calls = []

    def build():
        calls.append(1)
        with torch.no_grad():
            m.weight[:, :, 2].zero_()
        return object()
    first = m._packs._cached(ROLE, (m.weight,), build)
    assert m._packs._cached(ROLE, (m.weight,), build) is first and len(calls) == 1
    cc.inplace_no_grad(m, [m.weight])                     # ... but a write from outside afterwards still counts
    assert m._packs._cached(ROLE, (m.weight,), build) is not first and len(calls) == 2
    m._packs._cached(ROLE, (m.weight,), build)
    assert len(calls) == 2


def test_a_view_of_the_same_memory_with_another_shape_rebuilds():
    """`.data` rebound to a reshaped view: same address, same version counter, same epoch -- the shape alone tells"""
    m, build = _conv(), Build()
    first = m._packs._cached(ROLE, (m.weight,), build)
    ptr, version = m.weight.data_ptr(), m.weight._version
    m.weight.data = m.weight.data.view(4, 4, 1, 9)
    assert (m.weight.data_ptr(), m.weight._version) == (ptr, version)
    second = m._packs._cached(ROLE, (m.weight,), build)
    assert second is not first and build.calls == 2
    assert m._packs._cached(ROLE, (m.weight,), build) is second


# ----------------------------------------------------------------------------- the fused schedule's key
#: mutations that write the chosen parameter only (the state-dict and whole-buffer ones rewrite every parameter with equal values,
#: which is a write all the same)
_TARGETED = ("inplace_no_grad", "copy_from_new", "sgd_foreach_on", "sgd_foreach_off", "adam_step", "rebind_data", "data_mul_bump_params")


def _stem():
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    return cc.make(SpatioTemporalPriorModel_Res, 64, 96)


@pytest.mark.parametrize("layer", ["context_prediction", "HD.0", "EPM.2"])
@pytest.mark.parametrize("name", [n for n in cc.CPU_MUTATIONS if n != "load_state_dict_assign"])
def test_engine_weights_key_changes_with_one_layers_weight(name, layer):
    """(the models' load_state_dict has the reference's signature: no `assign`)"""
    mutate = cc.CPU_MUTATIONS[name]
    m = _stem()
    cc.prepare(mutate, m)
    eng = m.engine()
    mods = [l.mod for l in eng.layers]
    idx = mods.index(m.get_submodule(layer))
    key = eng._weights_key()
    assert eng._weights_key() == key                      # an untouched model: the same key
    mutate(m, cc.lookup(m, [layer + ".weight"]))
    after = eng._weights_key()
    assert after[idx] != key[idx], f"{name}: the key missed the change of {layer}.weight"
    if name in _TARGETED:
        assert [i for i in range(len(key)) if after[i] != key[i]] == [idx]
    assert eng._weights_key() == after


def test_engine_weights_key_data_write_and_bump():
    m = _stem()
    eng = m.engine()
    key = eng._weights_key()
    cc.STALE_MUTATION(m, [m.EPM[2].weight])
    assert eng._weights_key() == key                      # the documented blind spot
    bump_weight_epoch([m.EPM[2].weight])
    after = eng._weights_key()
    idx = [l.mod for l in eng.layers].index(m.EPM[2])
    assert [i for i in range(len(key)) if after[i] != key[i]] == [idx]
    bump_weight_epoch()
    assert all(a != b for a, b in zip(eng._weights_key(), after))


# ----------------------------------------------------------------------------- host CDF tables
class _Holder(torch.nn.Module):
    def __init__(self, channels=4):
        super().__init__()
        from spatiotemporalentropymodel_amd.entropy_models import EntropyBottleneck
        self.entropy_bottleneck = EntropyBottleneck(channels)


@pytest.mark.parametrize("name", ["inplace_no_grad", "copy_from_new", "rebind_data", "sgd_foreach_off"])
def test_host_tables_follow_update(name):
    eb = cc.make(_Holder).entropy_bottleneck
    assert eb.update(force=True)
    t = eb.host_tables()
    assert eb.host_tables() is t
    cdf = eb._quantized_cdf.clone()
    cc.CPU_MUTATIONS[name](eb, list(eb.parameters()))
    assert eb.host_tables() is t                          # the tables are a function of update(), not of the parameters
    assert eb.update(force=True)
    assert not (cdf.shape == eb._quantized_cdf.shape and torch.equal(cdf, eb._quantized_cdf)), "the mutation did not change the tables"
    t2 = eb.host_tables()
    assert t2 is not t
    assert eb.host_tables() is t2


def test_host_tables_follow_load_state_dict():
    a, b = cc.make(_Holder), cc.make(_Holder)
    a.entropy_bottleneck.update(force=True)
    with torch.no_grad():
        b.entropy_bottleneck._bias0.add_(0.75)            # same table size, other masses
    b.entropy_bottleneck.update(force=True)
    assert a.entropy_bottleneck._quantized_cdf.shape == b.entropy_bottleneck._quantized_cdf.shape
    assert not torch.equal(a.entropy_bottleneck._quantized_cdf, b.entropy_bottleneck._quantized_cdf)
    t = a.entropy_bottleneck.host_tables()
    a.load_state_dict(b.state_dict())
    t2 = a.entropy_bottleneck.host_tables()
    assert t2 is not t and a.entropy_bottleneck.host_tables() is t2
    assert torch.equal(a.entropy_bottleneck._quantized_cdf, b.entropy_bottleneck._quantized_cdf)


def test_host_tables_follow_a_load_state_dict_that_resizes():
    from spatiotemporalentropymodel_amd.models.utils import update_registered_buffers
    a, b = cc.make(_Holder), cc.make(_Holder)
    a.entropy_bottleneck.update(force=True)
    with torch.no_grad():
        b.entropy_bottleneck.quantiles.mul_(2.0)          # wider distributions: longer tables
    b.entropy_bottleneck.update(force=True)
    assert a.entropy_bottleneck._quantized_cdf.shape != b.entropy_bottleneck._quantized_cdf.shape
    t = a.entropy_bottleneck.host_tables()
    sd = b.state_dict()
    update_registered_buffers(a.entropy_bottleneck, "entropy_bottleneck", ["_quantized_cdf", "_offset", "_cdf_length"], sd, policy="resize")
    a.load_state_dict(sd)
    t2 = a.entropy_bottleneck.host_tables()
    assert t2 is not t and a.entropy_bottleneck.host_tables() is t2
    assert tuple(a.entropy_bottleneck._quantized_cdf.shape) == tuple(b.entropy_bottleneck._quantized_cdf.shape)


def test_host_tables_follow_buffers_that_were_replaced_or_reshaped():
    """load_state_dict(assign=True) puts the donor's tensors in place of the buffers: never written (version 0 like the old ones),
    the same shape -- the address alone tells.  `.data` rebound to a narrower view of the same memory: the shape alone tells."""
    import inspect
    a, b = cc.make(_Holder), cc.make(_Holder)
    a.entropy_bottleneck.update(force=True)
    with torch.no_grad():
        b.entropy_bottleneck._bias0.add_(0.75)
    b.entropy_bottleneck.update(force=True)
    eb = a.entropy_bottleneck
    t = eb.host_tables()
    if "assign" in inspect.signature(torch.nn.Module.load_state_dict).parameters:
        old = (eb._quantized_cdf._version, tuple(eb._quantized_cdf.shape))
        a.load_state_dict(b.state_dict(), assign=True)
        eb = a.entropy_bottleneck
        assert (eb._quantized_cdf._version, tuple(eb._quantized_cdf.shape)) == old
        t2 = eb.host_tables()
        assert t2 is not t and (t2.cdf != t.cdf).any()
        t = t2
    ptr, version = eb._quantized_cdf.data_ptr(), eb._quantized_cdf._version
    eb._quantized_cdf.data = eb._quantized_cdf.data[:, :-1]
    assert (eb._quantized_cdf.data_ptr(), eb._quantized_cdf._version) == (ptr, version)
    t3 = eb.host_tables()
    assert t3 is not t and t3.cdf.shape[1] == t.cdf.shape[1] - 1
