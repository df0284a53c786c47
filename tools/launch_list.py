#!/usr/bin/env python3
"""The canonical launch list of the layer-wise paths and the codec: which library entry points a set of scenarios calls, in order, with
every argument that is not an address.  Dev tool for refactors of layers.py / engine.py / codec.py that must not change a launch: run it at the
parent commit and at the new one and `diff` the two files.

    python tools/launch_list.py OUT.txt [scenario-name-prefix ...]

One line per launch: entry point, then the non-address arguments (integers as they are, floats by bit pattern); for the `*_multi`
entry points the non-address fields of every descriptor follow.  Every scenario is listed twice: first call (weights are packed)
and second call (packs cached).  Built on tape.recording(), which sees every int-returning call that goes through _lib.hip()."""
import ctypes as C
import os
import struct
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from spatiotemporalentropymodel_amd import _lib, config, tape  # noqa: E402


class ListTape(tape.LaunchTape):
    """add_call writes the canonical line instead of a replayable entry"""

    def __init__(self):
        super().__init__()
        self.lines = []

    def add_call(self, name, fn, args):
        out = [name]
        for a, ty in zip(args, _lib._HIP_SIG[name]):
            if ty is C.c_void_p:
                if isinstance(a, C.Array) and issubclass(a._type_, C.Structure):
                    for d in a:
                        out.append("{" + ",".join(str(getattr(d, f)) for f, fty in d._fields_ if fty is not C.c_void_p) + "}")
            elif ty is C.c_float:
                out.append("f" + struct.pack("<f", float(a)).hex())
            elif ty is C.c_double:
                out.append("d" + struct.pack("<d", float(a)).hex())
            else:
                out.append(str(int(a)))
        self.lines.append(" ".join(out))

    def bind_floats(self, provider):        # the optimiser's replay hook: nothing is replayed here
        pass


def listed(fn):
    t = ListTape()
    with tape.recording(t, keep_allocations=False):
        fn()
    torch.cuda.synchronize()
    return t.lines


DEV = torch.device("cuda:0")
SCENARIOS = []


def scenario(name, **cfg):
    """the decorated function builds the scenario (models are new: the first call packs) and returns the callable listed twice"""
    def deco(make):
        SCENARIOS.append((name, cfg, make))
        return make
    return deco


def _mbt(N=None, M=None):
    from spatiotemporalentropymodel_amd.models.priors import JointAutoregressiveHierarchicalPriors
    from spatiotemporalentropymodel_amd.zoo import models
    torch.manual_seed(5)
    m = models["mbt2018"](quality=4) if N is None else JointAutoregressiveHierarchicalPriors(N, M)
    return m.to(DEV).eval()


def _fwd_bwd(net, x, grad):
    def run():
        if not grad:
            with torch.no_grad():
                return net(x)
        y = net(x.requires_grad_(x.shape[1] != 3))      # the image needs no gradient
        y.backward(torch.ones_like(y))
    return run


for shape in ((16, 3, 256, 256), (2, 3, 256, 256), (1, 3, 1088, 1920)):
    for a in (True, False):
        for c in (True, False):
            scenario(f"g_a nograd {shape} analysis={int(a)} first={int(c)}", analysis_f16x3=a, first_layer_f16x3=c)(
                lambda shape=shape: _fwd_bwd(_mbt().g_a, torch.rand(shape, device=DEV), False))
scenario("g_a autograd (16, 3, 256, 256)")(lambda: _fwd_bwd(_mbt().g_a, torch.rand(16, 3, 256, 256, device=DEV), True))
for N, M in ((128, 192), (192, 320)):
    for B, H in ((2, 16), (8, 64)):
        for part, ch, div in (("g_s", M, 1), ("h_a", M, 1), ("h_s", N, 4), ("entropy_parameters", 4 * M, 1)):
            for grad in (False, True):
                scenario(f"{part} ({N},{M}) B={B} H={H // div} {'autograd' if grad else 'nograd'}")(
                    lambda N=N, M=M, B=B, H=H, part=part, ch=ch, div=div, grad=grad:
                    _fwd_bwd(getattr(_mbt(N, M), part), torch.rand(B, ch, H // div, H // div, device=DEV), grad))


def _roi_iteration():
    """I(x0, Q) then P(x1, x_hat_I, Q), both back-propagated into FlatParameters (tests/test_hip_roi.py)"""
    from spatiotemporalentropymodel_amd.losses import PixelwiseRateDistortionLoss, quality2lambda
    from spatiotemporalentropymodel_amd.models import stem_roi, stem_roi_i
    from spatiotemporalentropymodel_amd.optim import configure_optimizers
    from spatiotemporalentropymodel_amd.selfcheck import NoiseFeed
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_scaled_, smooth_frames
    g = np.load(os.path.join(REPO, "tests", "golden", "stem_roi.npz"))
    B, size = (int(v) for v in g["cfg"])
    ms, opts = [], []
    args = types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3)
    for tag, cls in (("roi_i", stem_roi_i), ("roi_p", stem_roi)):
        m = closed_form_fill_scaled_(cls(), tag, 0.7).to(DEV).train()
        m.entropy_bottleneck.noise_source = NoiseFeed(tag + "_eb")
        m.gaussian_conditional.noise_source = NoiseFeed(tag + "_gc")
        ms.append(m)
        opts += configure_optimizers(m, args, max_norm=None)
    frames = [f.to(DEV) for f in smooth_frames("roi", B, 2, size)]
    qmap = torch.from_numpy(g["qmap"]).to(DEV)
    lmbdamap, crit = quality2lambda(qmap), PixelwiseRateDistortionLoss()

    def run():
        for o in opts:
            o.zero_grad()
        out_i = ms[0](frames[0], qmap)
        crit(out_i, frames[0], lmbdamap)["loss"].backward(retain_graph=True)
        out_p = ms[1](frames[1], out_i["x_hat"], qmap)
        crit(out_p, frames[1], lmbdamap)["loss"].backward()
    return run


for on in (True, False):
    for wide in (None, 0):
        for maxpix in (None, 0):
            cfg = dict(layers_f16x3=on, **({} if wide is None else {"layers_wide_minpix": wide}),
                       **({} if maxpix is None else {"layers_f16x3_maxpix": maxpix}))
            scenario(f"roi I+P training f16x3={int(on)} wide_minpix={wide} maxpix={maxpix}", **cfg)(_roi_iteration)


@scenario("mbt2018 compress + decompress")
def _codec():
    from spatiotemporalentropymodel_amd.models.priors import JointAutoregressiveHierarchicalPriors
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    g = np.load(os.path.join(REPO, "tests", "golden", "iframe_codec_small.npz"))
    m = closed_form_fill_(JointAutoregressiveHierarchicalPriors(64, 96)).to(DEV).eval()
    m.update(force=True)
    x = torch.from_numpy(g["x"]).to(DEV)

    def run():
        enc = m.compress(x)
        m.decompress(enc["strings"], enc["shape"])
    return run


def _stem_codec(cls_name, B):
    """compress() then decompress() of a [B, 96, 8, 12] latent; the persistent decoder's once-per-process self-check is forgotten
    first, so each scenario's first call lists it at the moment its route asks for it"""
    import spatiotemporalentropymodel_amd.models as M
    from spatiotemporalentropymodel_amd import codec
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_, closed_form_input
    m = closed_form_fill_(getattr(M, cls_name)(64, 96)).to(DEV).eval()
    m.update(force=True)
    y_cur = closed_form_input("ll:y", (B, 96, 8, 12), -6, 6).to(DEV)
    y_cond = closed_form_input("ll:c", (B, 96, 8, 12), -6, 6).to(DEV)
    codec._ARP_TRUSTED.clear()

    def run():
        with torch.no_grad():
            enc = m.compress(y_cur, y_cond)
            m.decompress(enc["strings"], enc["shape"], y_cond)
    return run


# every form of the decoder's loop (codec.decode_route); B=3 with the defaults issues its launches from worker threads: compare
# that scenario's lines sorted
for cls_name in ("SpatioTemporalPriorModel_Res", "SpatioTemporalPriorModelWithoutTPM"):
    for B, cfg in ((1, {}), (1, {"ar_persistent": False}), (1, {"ar_stepwise": True}), (1, {"ar_force_batch": True}),
                   (3, {}), (3, {"ar_concurrent": False}), (3, {"ar_no_batch": True, "ar_persistent": False})):
        scenario(f"STEM codec {cls_name} B={B} {cfg}", **cfg)(lambda cls_name=cls_name, B=B: _stem_codec(cls_name, B))


@scenario("STEM P-frame step, small geometry")
def _pframe():
    from spatiotemporalentropymodel_amd import selfcheck as S
    from spatiotemporalentropymodel_amd.optim import configure_optimizers
    from spatiotemporalentropymodel_amd.trainer import FusedPFrameStep
    torch.manual_seed(11)
    imodel, stem = S.build_models(64, 96, 64, 96, DEV, closed_form=False, inject_noise=False)
    stem.train()
    fused = FusedPFrameStep(stem, *configure_optimizers(stem, types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3)))
    gen = torch.Generator(device=DEV).manual_seed(2)
    frames = [torch.rand(2, 3, 128, 128, device=DEV, generator=gen) for _ in range(2)]

    def run():
        with torch.no_grad():
            y_cond, y_cur = imodel.getY(frames[0])[1], imodel.getY(frames[1])[0]
        fused.step(y_cur, y_cond, 2 * 128 * 128)
        fused.finish()
    return run


def main():
    out_path, prefixes = sys.argv[1], tuple(sys.argv[2:])
    with open(out_path, "w") as out:
        for name, cfg, make in SCENARIOS:
            if prefixes and not name.startswith(prefixes):
                continue
            with config.override(**cfg):
                run = make()
                for call in ("first", "second"):
                    lines = listed(run)
                    out.write(f"== {name} | {call} call | {len(lines)} launches\n" + "".join(l + "\n" for l in lines))
                    print(f"{name} | {call} call | {len(lines)} launches", flush=True)
            out.flush()


if __name__ == "__main__":
    main()
