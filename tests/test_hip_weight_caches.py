"""GPU: no kernel reads a `weight`; it reads a packed copy (layers._PackCache, engine.ensure_packed), a host CDF table
(EntropyModel.host_tables) or a recorded launch (tape.TapedPFrameStep) made earlier.  Every test here follows one pattern:

    run the subject once (warm caches)  ->  change parameters  ->  run again  ->  run a twin that has never run

and requires the second run to EQUAL the twin's, bit for bit (same plan, same kernels, and the suite holds relaunches
bit-identical: no tolerance anywhere), and to DIFFER from the first run.  The planned route is asserted before anything runs, so
a threshold change cannot move a case onto another kernel unnoticed.  tests/cache_cases.py has the mutations, the twin and the
pack counters; tests/test_weight_caches.py holds the host-side keys alone.

What is compared: y, dx, dw, db of the layer-wise subjects (so the _FLIP / _DGRAD roles are held, not only the forward pack); the
output of the inference chains; y_hat, the likelihoods, every parameter gradient, the eval forward and the bitstreams of the fused
schedule.  The loss scalars of the training step (stem_log2_sum, stem_weighted_sqerr_sum, stem_eb_aux_loss) pass through a float
atomic accumulation and are not compared: the tensors in front of them are.

"Differs from the first run" is asked of the tensors the changed parameters reach: y and dx of a convolution.  Its dw = x (*) dy
and db = sum dy do not contain the weight at all."""
import pytest
import torch

import cache_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _layers():
    from spatiotemporalentropymodel_amd import layers
    return layers


def _cfg():
    from spatiotemporalentropymodel_amd import config
    return config.runtime()


def _det(shape, salt=0.0):
    """a deterministic tensor of `shape` (NHWC memory for 4-D) with values in [-1, 1]"""
    n = 1
    for s in shape:
        n *= s
    t = torch.sin(torch.arange(n, device=DEV, dtype=torch.float32) * 0.37 + salt).view(shape)
    return t.contiguous(memory_format=torch.channels_last) if len(shape) == 4 else t


def _image(shape):
    return (_det(shape) * 0.5 + 0.5).contiguous()


def _on_dev(m):
    return m.to(DEV)


# ----------------------------------------------------------------------------- subjects
class Subject:
    """module factory, input, the parameters a mutation moves, the routes the plan must give, and how to run it"""

    def __init__(self, build, x_shape, params, routes, infer=False, image=False):
        self.build, self.x_shape, self.params, self.routes, self.infer, self.image = build, x_shape, params, routes, infer, image

    def module(self):
        torch.manual_seed(5)
        return _on_dev(self.build())

    def x(self):
        return _image(self.x_shape) if self.image else _det(self.x_shape, 1.0).contiguous()

    def planned(self, m):
        L = _layers()
        if isinstance(m, L.FusedSequential):
            return [str(s.route) for s in m.plan(self.x_shape, "nchw", not self.infer, True) if s.route is not None]
        r = L.route(m, self.x_shape, "nchw", grad=True, on_device=True)
        return [f"{r}/{r.dgrad}"]

    def run(self, m):
        """-> the compared tensors: [y] under no_grad, [y, dx, dw, db, ...] layer-wise"""
        x = self.x()
        if self.infer:
            with torch.no_grad():
                return [m(x).clone()]
        xg = x.requires_grad_(True)
        y = m(xg)
        grads = torch.autograd.grad(y, [xg] + list(m.parameters()), _det(tuple(y.shape), 2.0))
        torch.cuda.synchronize()
        return [y.detach().clone()] + [g.clone() for g in grads]


def _wide_hw():
    """the first pixel count at or above layers_wide_minpix, as 128 rows"""
    minpix = _cfg().layers_wide_minpix
    return 128, -(-minpix // 128)


def _chain_image():
    """an image whose second stride-2 layer has exactly _F16X3_MIN_PIXELS output pixels (1 x 3 x 512 x 384 at 12288)"""
    minpix = _layers()._F16X3_MIN_PIXELS
    assert minpix % 128 == 0
    return (1, 3, 4 * 128, 4 * (minpix // 128))


def _subjects():
    L = _layers()
    mk = cc.make
    conv3 = lambda cin, cout: mk(L.Conv2d, cin, cout, 3, padding=1)
    c4h_width = min(k for k in (64, 128, 192) if _c4gdn_supported(k))
    chain = lambda: mk(L.FusedSequential, mk(L.Conv2d, 3, c4h_width, 5, stride=2, padding=2), mk(L.GDN, c4h_width),
                       mk(L.Conv2d, c4h_width, 64, 5, stride=2, padding=2), mk(L.GDN, 64), mk(L.Conv2d, 64, 64, 5, stride=2, padding=2))
    Hw, Ww = _wide_hw()
    chain_routes = ["c4h+gdn -> planes", "wide+gdn -> planes", "gen"]
    return {
        # layer-wise autograd routes ("forward family/input-gradient family")
        "f32": Subject(lambda: conv3(33, 8), (1, 33, 8, 8), ["weight", "bias"], ["f32/f32"]),
        "c4": Subject(lambda: mk(L.Conv2d, 3, 8, 5, stride=2, padding=2), (1, 3, 16, 16), ["weight", "bias"], ["c4/f32"]),
        "gen": Subject(lambda: conv3(64, 64), (1, 64, 16, 16), ["weight", "bias"], ["gen/gen"]),
        "wide": Subject(lambda: conv3(64, 64), (1, 64, Hw, Ww), ["weight", "bias"], ["wide/wide"]),
        "deconv": Subject(lambda: mk(L.ConvTranspose2d, 8, 8, 5, stride=2, padding=2, output_padding=1), (1, 8, 5, 7), ["weight", "bias"], ["f32/f32"]),
        "deconv_rgb": Subject(lambda: mk(L.ConvTranspose2d, 8, 3, 5, stride=2, padding=2, output_padding=1), (1, 8, 5, 7), ["weight", "bias"], ["f32/f32"]),
        "masked_A": Subject(lambda: mk(L.MaskedConv2d, 8, 16, 5, padding=2, mask_type="A"), (1, 8, 6, 7), ["weight"], ["f32/f32"]),
        "masked_B": Subject(lambda: mk(L.MaskedConv2d, 8, 16, 5, padding=2, mask_type="B"), (1, 8, 6, 7), ["weight"], ["f32/f32"]),
        "pair_second": Subject(lambda: mk(L.FusedSequential, conv3(64, 64), mk(L.LeakyReLU, 0.01), conv3(64, 64)), (1, 64, 16, 16),
                               ["2.weight", "2.bias"], ["gen -> planes", "gen"]),
        # inference routes, under no_grad through FusedSequential
        "c4h_weight": Subject(lambda: mk(L.FusedSequential, mk(L.Conv2d, 3, c4h_width, 5, stride=2, padding=2), mk(L.GDN, c4h_width)),
                              (1, 3, 16, 16), ["0.weight"], ["c4h+gdn"], infer=True, image=True),
        "c4h_gamma": Subject(lambda: mk(L.FusedSequential, mk(L.Conv2d, 3, c4h_width, 5, stride=2, padding=2), mk(L.GDN, c4h_width)),
                             (1, 3, 16, 16), ["1.gamma"], ["c4h+gdn"], infer=True, image=True),
        "c4h_beta": Subject(lambda: mk(L.FusedSequential, mk(L.Conv2d, 3, c4h_width, 5, stride=2, padding=2), mk(L.GDN, c4h_width)),
                            (1, 3, 16, 16), ["1.beta"], ["c4h+gdn"], infer=True, image=True),
        "chain_c4h_weight": Subject(chain, _chain_image(), ["0.weight"], chain_routes, infer=True, image=True),
        "chain_c4h_gamma": Subject(chain, _chain_image(), ["1.gamma"], chain_routes, infer=True, image=True),
        "chain_wide_gamma": Subject(chain, _chain_image(), ["3.gamma"], chain_routes, infer=True, image=True),     # PACK_GDN_GAMMA, in conv 2's cache
        "chain_wide_weight": Subject(chain, _chain_image(), ["2.weight"], chain_routes, infer=True, image=True),
        "chain_gen_tail": Subject(chain, _chain_image(), ["4.weight"], chain_routes, infer=True, image=True),
        "f32_gdn": Subject(lambda: mk(L.FusedSequential, conv3(8, 8), mk(L.GDN, 8)), (1, 8, 8, 8), ["0.weight"], ["f32+gdn"], infer=True),
        "deconv_igdn": Subject(lambda: mk(L.FusedSequential, mk(L.ConvTranspose2d, 8, 8, 5, stride=2, padding=2, output_padding=1),
                                          mk(L.GDN, 8, inverse=True)), (1, 8, 5, 7), ["0.weight"], ["f32+gdn"], infer=True),
    }


def _c4gdn_supported(k):
    from spatiotemporalentropymodel_amd import functional as F
    return F.c4gdn_supported(k, 5, 5)


SUBJECTS = ["f32", "c4", "gen", "wide", "deconv", "deconv_rgb", "masked_A", "masked_B", "pair_second", "c4h_weight", "c4h_gamma", "c4h_beta",
            "chain_c4h_weight", "chain_c4h_gamma", "chain_wide_gamma", "chain_wide_weight", "chain_gen_tail", "f32_gdn", "deconv_igdn"]
#: the chains run ~50k pixels: they take the mutations that reach a key in different ways, the small subjects take every one
_CHAIN_MUTATIONS = ("inplace_no_grad", "load_state_dict_", "rebind_data", "data_mul_bump_params", "flat_restore")


def _cases():
    out = []
    for s in SUBJECTS:
        for name in cc.MUTATIONS:
            if s.startswith("chain_") and name not in _CHAIN_MUTATIONS:
                continue
            out.append((s, name))
    return out


def _same(a, b):
    return len(a) == len(b) and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(a, b))


def _reached(subject, outs):
    """the compared tensors the changed parameters reach: y, and dx of the layer-wise runs"""
    return outs[:1] if subject.infer else outs[:2]


@pytest.mark.parametrize("subject,mutation", _cases())
def test_next_launch_sees_the_change(subject, mutation):
    s, mutate = _subjects()[subject], cc.MUTATIONS[mutation]
    m = s.module()
    assert s.planned(m) == s.routes
    cc.prepare(mutate, m)
    first = s.run(m)
    assert _same(first, s.run(m)), "two runs of unchanged parameters differ: the comparison below would mean nothing"
    mutate(m, cc.lookup(m, s.params))
    second = s.run(m)
    other = cc.twin(m)
    assert s.planned(other) == s.routes
    want = s.run(other)
    for i, (a, b) in enumerate(zip(second, want)):
        assert torch.equal(a, b), f"{subject} after {mutation}: compared tensor {i} is not what a model that never ran computes"
    for i, (a, b) in enumerate(zip(_reached(s, second), _reached(s, first))):
        assert not torch.equal(a, b), f"{subject} after {mutation}: compared tensor {i} did not change at all"


@pytest.mark.parametrize("subject", ["f32", "gen", "deconv", "masked_A", "c4h_weight", "c4h_gamma", "chain_wide_gamma", "f32_gdn"])
def test_data_write_is_stale_until_the_epoch_is_bumped(subject):
    """INTEGRATION.md, "Writing weights through .data": the one change nobody can see.  Without bump_weight_epoch the next launch
    computes with the OLD copies (asserted: it is the documented behaviour, and a key that began to see such writes would be a
    change of contract); with it, with the new values."""
    from spatiotemporalentropymodel_amd.layers import bump_weight_epoch
    s = _subjects()[subject]
    names = [n for n in s.params if not n.endswith("bias")]          # the bias is read where it lies: it has no copy to go stale
    m = s.module()
    assert s.planned(m) == s.routes
    first = s.run(m)
    cc.STALE_MUTATION(m, cc.lookup(m, names))
    stale = s.run(m)
    for a, b in zip(_reached(s, stale), _reached(s, first)):
        assert torch.equal(a, b)
    bump_weight_epoch(cc.lookup(m, names))
    second, want = s.run(m), s.run(cc.twin(m))
    assert _same(second, want)
    for a, b in zip(_reached(s, second), _reached(s, first)):
        assert not torch.equal(a, b)


@pytest.mark.parametrize("mask_type", ["A", "B"])
def test_masked_tap_written_from_outside_is_zeroed_again(mask_type, monkeypatch):
    """the pack zeroes the masked taps of `weight` in place at every forward that packs.  A masked tap set to non-zero (a visible
    write) is zero again after the next forward, the output is a never-run model's, and equal to the output before the write (a
    masked tap reaches nothing); two forwards in a row pack once."""
    s = _subjects()["masked_" + mask_type]
    m = s.module()
    counts = cc.count_packs(monkeypatch)
    x = s.x()
    with torch.no_grad():
        first = m(x).clone()
        assert counts.total() == 1 and counts["pack_weight"] == 1
        m(x)
        assert counts.total() == 1
        assert bool((m.weight * (1 - m.mask) == 0).all())
        m.weight[:, :, 4, 4] = 0.3
        assert not bool((m.weight * (1 - m.mask) == 0).all())
        other = cc.twin(m)
        second = m(x).clone()
        assert counts.total() == 2
        assert bool((m.weight * (1 - m.mask) == 0).all()), "the masked taps were not zeroed by the forward that packed"
        assert torch.equal(second, other(x)) and torch.equal(second, first)
        m(x)
        assert counts.total() == 3                      # (the twin's own pack was the third)


# ----------------------------------------------------------------------------- no needless packs
def test_unchanged_weights_cost_no_pack_layerwise_and_only_the_changed_layer_repacks(monkeypatch):
    L = _layers()
    mk = cc.make
    torch.manual_seed(5)
    m = _on_dev(mk(L.FusedSequential, mk(L.Conv2d, 64, 64, 3, padding=1), mk(L.LeakyReLU, 0.01), mk(L.Conv2d, 64, 64, 3, padding=1),
                   mk(L.LeakyReLU, 0.01), mk(L.Conv2d, 64, 64, 3, padding=1)))
    s = Subject(None, (1, 64, 16, 16), ["2.weight"], ["gen -> planes", "gen -> planes", "gen"])
    assert s.planned(m) == s.routes
    counts = cc.count_packs(monkeypatch)
    s.run(m)
    assert dict(counts) == {"PACK_F16X2_GEN": 3, "PACK_F16X2_GEN_FLIP": 3}
    counts.reset()
    s.run(m)
    assert counts.total() == 0, dict(counts)
    cc.inplace_no_grad(m, [m[2].weight])
    s.run(m)
    assert dict(counts) == {"PACK_F16X2_GEN": 1, "PACK_F16X2_GEN_FLIP": 1}
    assert set(counts.weights["PACK_F16X2_GEN"] + counts.weights["PACK_F16X2_GEN_FLIP"]) == {m[2].weight.data_ptr()}
    counts.reset()
    s.run(m)
    assert counts.total() == 0, dict(counts)


def test_unchanged_weights_cost_no_pack_inference_chain(monkeypatch):
    s = _subjects()["chain_wide_gamma"]
    m = s.module()
    assert s.planned(m) == s.routes
    counts = cc.count_packs(monkeypatch)
    s.run(m)
    assert counts.total() > 0 and counts["c4gdn_stream"] == 1 and counts["PACK_GDN_GAMMA"] == 1
    counts.reset()
    s.run(m)
    assert counts.total() == 0, dict(counts)
    cc.inplace_no_grad(m, [m[3].gamma])                  # the second GDN's gamma: one entry of the second convolution's cache
    s.run(m)
    assert dict(counts) == {"PACK_GDN_GAMMA": 1}


# ----------------------------------------------------------------------------- the fused schedule
def _stem():
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    m = closed_form_fill_(cc.make(SpatioTemporalPriorModel_Res, 64, 96)).to(DEV)
    m.update(force=True)
    return m


def _latents():
    from spatiotemporalentropymodel_amd.weights import closed_form_input
    return (closed_form_input("wc:y", (1, 96, 8, 20), -6, 6).to(DEV), closed_form_input("wc:c", (1, 96, 8, 20), -6, 6).to(DEV))


def _stem_train(m, y_cur, y_cond):
    """training forward and backward -> [y_hat, lik_y, lik_z, every parameter gradient]"""
    m.train()
    for e in (m.entropy_bottleneck, m.gaussian_conditional):
        e._noise_offset = 0                             # the same noise draw in every run
    params = [p for n, p in sorted(m.named_parameters()) if not n.endswith(".quantiles")]
    for p in params:
        view = getattr(p, "_flat_grad_view", None)
        if view is not None:
            view.zero_()
        p.grad = None
    out = m(y_cur, y_cond)
    lik_y, lik_z = out["likelihoods"]["y"], out["likelihoods"]["z"]
    torch.autograd.backward([lik_y, lik_z], [_det(tuple(lik_y.shape), 3.0), _det(tuple(lik_z.shape), 4.0)])
    torch.cuda.synchronize()
    grads = [p.grad.clone() if p.grad is not None else torch.zeros_like(p) for p in params]
    return [out["y_hat"].detach().clone(), lik_y.detach().clone(), lik_z.detach().clone()] + grads


def _stem_eval(m, y_cur, y_cond):
    m.eval()
    with torch.no_grad():
        out = m(y_cur, y_cond)
    return [out["y_hat"].clone(), out["likelihoods"]["y"].clone(), out["likelihoods"]["z"].clone()]


def _stem_code(m, y_cur, y_cond):
    m.eval()
    with torch.no_grad():
        enc = m.compress(y_cur, y_cond)
        dec = m.decompress(enc["strings"], enc["shape"], y_cond)
    return enc["strings"], dec["y_hat"].clone()


_STEM_LAYERS = ["context_prediction", "HD.0", "EPM.2"]


def _stem_cases():
    names = [n for n in cc.MUTATIONS if n != "load_state_dict_assign"]          # the models' load_state_dict has no `assign`
    return [("EPM.2", n) for n in names] + [(l, n) for l in _STEM_LAYERS[:2] for n in ("inplace_no_grad", "rebind_data", "flat_restore")]


@pytest.mark.parametrize("layer,mutation", _stem_cases())
def test_fused_schedule_sees_one_layers_change(layer, mutation):
    """STEM at the widths of tests/test_hip_codec.py, (64, 96) latents of 8 x 20: the masked context weight, a transposed
    hyper-decoder layer, one 1x1 entropy-parameter layer, one at a time"""
    mutate = cc.MUTATIONS[mutation]
    m = _stem()
    cc.prepare(mutate, m)
    y_cur, y_cond = _latents()
    first = (_stem_train(m, y_cur, y_cond), _stem_eval(m, y_cur, y_cond), _stem_code(m, y_cur, y_cond))
    mutate(m, cc.lookup(m, [layer + ".weight"]))
    second = (_stem_train(m, y_cur, y_cond), _stem_eval(m, y_cur, y_cond), _stem_code(m, y_cur, y_cond))
    other = cc.twin(m)
    want = (_stem_train(other, y_cur, y_cond), _stem_eval(other, y_cur, y_cond), _stem_code(other, y_cur, y_cond))
    for i, (a, b) in enumerate(zip(second[0], want[0])):
        assert torch.equal(a, b), f"training pass after {mutation} of {layer}: tensor {i} (y_hat, lik_y, lik_z, then the gradients by name)"
    assert _same(second[1], want[1]), "eval forward"
    assert second[2][0] == want[2][0], "bitstreams"
    assert torch.equal(second[2][1], want[2][1]), "decoded latents"
    # every layer reaches the latents' likelihoods (and through them the coded bytes)
    assert not torch.equal(second[0][1], first[0][1]) and not torch.equal(second[1][1], first[1][1])
    assert second[2][0][0] != first[2][0][0]


def test_fused_schedule_data_write_is_stale_until_the_epoch_is_bumped():
    from spatiotemporalentropymodel_amd.layers import bump_weight_epoch
    m = _stem()
    y_cur, y_cond = _latents()
    first = _stem_eval(m, y_cur, y_cond)
    cc.STALE_MUTATION(m, [m.HD[0].weight])
    assert _same(_stem_eval(m, y_cur, y_cond), first)    # documented: INTEGRATION.md, "Writing weights through .data"
    bump_weight_epoch()
    second = _stem_eval(m, y_cur, y_cond)
    assert _same(second, _stem_eval(cc.twin(m), y_cur, y_cond)) and not torch.equal(second[1], first[1])


def test_fused_schedule_packs_once_per_change(monkeypatch):
    """two forwards and backwards with nothing changed: the second packs nothing.  One weight changed: ensure_packed issues the
    launches of one cold pass, the next forward none.  After FusedClipAdam.step(block_max=True): the pair pack, once."""
    from spatiotemporalentropymodel_amd.optim import FusedClipAdam
    m = _stem()
    flat = cc.flat_of(m)
    y_cur, y_cond = _latents()
    counts = cc.count_packs(monkeypatch)
    multi = ("pack_weights_multi", "pack_weights_f16x2_multi", "pack_weights_f16x2_pair_multi")
    _stem_train(m, y_cur, y_cond)
    cold = dict(counts)
    assert sum(cold.values()) > 0 and set(cold) <= set(multi[:2]), cold
    counts.reset()
    unchanged = _stem_train(m, y_cur, y_cond)
    assert counts.total() == 0, dict(counts)
    cc.inplace_no_grad(m, [m.EPM[2].weight])
    _stem_train(m, y_cur, y_cond)
    assert dict(counts) == cold
    counts.reset()
    changed = _stem_train(m, y_cur, y_cond)
    assert counts.total() == 0, dict(counts)
    assert not torch.equal(changed[1], unchanged[1])
    # The optimiser pass that leaves chunk maxima: the next ensure_packed takes the pair-pack path.  Its fp16 images are scaled by a
    # BOUND of max |w| (the maxima of the optimiser's chunks that cover the weight, which reach into its neighbours) where a cold
    # pack measures the maximum itself: the low planes differ, so the oracle here is a twin that has never run and goes the same
    # way -- loaded before the step, given the same gradients, stepped and packed by the same calls.
    other = cc.twin(m)
    flat_o = cc.flat_of(other)
    flat_o.grad.copy_(flat.grad)

    def step_and_pack(model, fl):
        opt = FusedClipAdam(fl, 1e-3)
        opt.step(block_max=True)
        model.engine().ensure_packed(block_max=(opt.block_maxima, fl.data))
    step_and_pack(m, flat)
    eng = m.engine()
    if eng.pack_pair and all(l.pair_desc() is not None for l in eng.layers):
        assert dict(counts) == {"pack_weights_f16x2_pair_multi": 1}
    else:
        assert counts.total() > 0
    counts.reset()
    after = _stem_train(m, y_cur, y_cond)
    assert counts.total() == 0, dict(counts)
    step_and_pack(other, flat_o)
    assert torch.equal(flat_o.data, flat.data)
    want = _stem_train(other, y_cur, y_cond)
    for i, (a, b) in enumerate(zip(after, want)):
        assert torch.equal(a, b), f"after FusedClipAdam.step(block_max=True): tensor {i}"
    assert not torch.equal(after[1], changed[1])


# ----------------------------------------------------------------------------- the recorded step
def test_taped_step_sees_a_checkpoint_loaded_between_two_replays(monkeypatch):
    """tape.TapedPFrameStep through two ordinary steps, two recorded and two replayed, with load_state_dict of a checkpoint taken
    after step 1 placed between the two replays: losses, latents and parameters equal the same sequence run untaped.  (The
    recorded step packs the weights at its end, for the next forward: a replay that follows a write must not read those copies.)"""
    from test_hip_trainer import _assert_same_run, _pair, _taped_run
    g = torch.Generator(device=DEV).manual_seed(23)
    frames = [torch.rand(2, 3, 128, 128, device=DEV, generator=g) for _ in range(7)]
    held = {}

    def make():
        held["models"] = _pair(64, 96, 64, 96, False, False)
        return held["models"]

    def edit(t, opt, aux):
        stem = held["models"][1]
        if t == 1:
            torch.cuda.synchronize()
            held["ckpt"] = {k: v.detach().clone() for k, v in stem.state_dict().items()}
        if t == 5:
            torch.cuda.synchronize()
            stem.load_state_dict(held["ckpt"])

    plain = _taped_run(False, 6, make, frames, 2 * 128 * 128, edit, monkeypatch=monkeypatch)
    taped = _taped_run(True, 6, make, frames, 2 * 128 * 128, edit, monkeypatch=monkeypatch)
    still = _taped_run(True, 6, make, frames, 2 * 128 * 128, None, monkeypatch=monkeypatch)
    assert taped[4].taped and taped[4].replays == 3 and taped[4].refused is None
    _assert_same_run(plain, taped)
    assert not torch.equal(still[0], taped[0])           # the load did change the run
    assert still[2][4][:4] == taped[2][4][:4] and still[2][5][:4] != taped[2][5][:4]


# ----------------------------------------------------------------------------- host CDF tables
def _image_model(kind):
    from spatiotemporalentropymodel_amd import models
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    cls = {"factorized": models.FactorizedPrior, "mean_scale": models.MeanScaleHyperprior}[kind]
    m = closed_form_fill_(cc.make(cls, 16, 16)).to(DEV).eval()
    m.update(force=True)
    return m


def _strings(m):
    return m.compress(_image((1, 3, 64, 64)))["strings"]


@pytest.mark.parametrize("mutation", ["inplace_no_grad", "copy_from_new", "rebind_data", "sgd_foreach_on"])
@pytest.mark.parametrize("kind", ["factorized", "mean_scale"])
def test_update_after_a_change_reaches_the_coder(kind, mutation):
    m = _image_model(kind)
    first = _strings(m)
    assert _strings(m) == first
    eb = m.entropy_bottleneck
    cc.MUTATIONS[mutation](eb, [eb._bias0, eb._bias1, eb.quantiles])
    assert m.update(force=True)
    second = _strings(m)
    other = cc.twin(m)
    assert other.update(force=True)
    assert second == _strings(other) and second != first


@pytest.mark.parametrize("kind", ["factorized", "mean_scale"])
def test_tables_loaded_from_another_model_reach_the_coder(kind):
    m, donor = _image_model(kind), _image_model(kind)
    first = _strings(m)
    with torch.no_grad():
        donor.entropy_bottleneck._bias0.add_(0.75)       # same table size, other masses
    donor.update(force=True)
    assert donor.entropy_bottleneck._quantized_cdf.shape == m.entropy_bottleneck._quantized_cdf.shape
    m.load_state_dict(donor.state_dict())
    second = _strings(m)
    assert second == _strings(cc.twin(m)) == _strings(donor) and second != first


# ----------------------------------------------------------------------------- the package's own writers
def test_closed_form_loader_reaches_the_kernels():
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_scaled_
    for subject in ("gen", "c4h_weight", "deconv"):
        s = _subjects()[subject]
        m = s.module()
        assert s.planned(m) == s.routes
        closed_form_fill_scaled_(m, "a", 0.7)
        first = s.run(m)
        closed_form_fill_scaled_(m, "b", 1.1)
        second = s.run(m)
        assert _same(second, s.run(cc.twin(m))), subject
        assert not torch.equal(second[0], first[0]), subject


@pytest.mark.parametrize("branch", ["staged", "direct"])
def test_broadcast_parameters_reaches_the_kernels_and_the_coder(branch, tmp_path, monkeypatch):
    """distributed.broadcast_parameters on a rank that has already run (a warm-up, a self-check): what it receives must be what
    the next launch and the coder use, with no help from the caller.  A world-size-1 gloo group on a file store; `broadcast` is
    replaced by what a receiving rank sees (the tensor it is handed filled with the source's values).  staged: through the host
    (gloo with device tensors); direct: the tensor itself (RCCL)."""
    import torch.distributed as dist
    from spatiotemporalentropymodel_amd.distributed import broadcast_parameters
    assert not dist.is_initialized()
    s = _subjects()["gen"]
    conv, model = s.module(), _image_model("factorized")
    source_conv, source_model = cc.twin(conv), cc.twin(model)
    with torch.no_grad():
        for p in source_conv.parameters():
            p.mul_(cc.FACTOR)
        source_model.g_a[0].weight.mul_(cc.FACTOR)
        source_model.entropy_bottleneck._bias0.add_(0.75)
    source_model.update(force=True)
    first = (s.run(conv), _strings(model))
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        for target, source in ((conv, source_conv), (model, source_model)):
            values = [t.detach() for t in list(source.parameters()) + list(source.buffers()) if t.numel()]
            handed = []

            def receive(tensor, src=0, **kwargs):
                handed.append(tensor.device.type)
                tensor.copy_(values[len(handed) - 1])
            monkeypatch.setattr(dist, "broadcast", receive)
            if branch == "direct":
                monkeypatch.setattr(dist, "get_backend", lambda *a, **k: "nccl")
            broadcast_parameters(target)
            assert len(handed) == len(values) and set(handed) == {"cpu" if branch == "staged" else "cuda"}
    finally:
        monkeypatch.undo()
        dist.destroy_process_group()
    second = (s.run(conv), _strings(model))
    assert _same(second[0], s.run(cc.twin(conv))) and _same(second[0], s.run(source_conv))
    assert second[1] == _strings(source_model)
    assert not torch.equal(second[0][0], first[0][0]) and second[1] != first[1]
