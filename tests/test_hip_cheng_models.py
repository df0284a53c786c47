"""GPU: the cheng2020 blocks and models against the reference's own runs (tests/golden/make_golden_cheng.py).

  cheng_blocks.npz          every block's output and every gradient against float64
  cheng_codec.<model>.npz   eval forward against float64; compress byte for byte; decompress of the reference's strings on both
                            decoder routes; wavefront order; batched coding
  cheng_gop.npz             evaluation.eval_gop with Cheng2020Anchor in front of a STEM P-frame model

Float64 gates are conftest.assert_close with rtol = max(1e-4, 3 x the reference's own fp32 distance from float64), the distance
taken from the fixture (the rule of tests/test_hip_spread.py).  The codec fixtures were chosen for their margins (how far the
nearest symbol is from a rounding / table threshold, in units of the reference's fp32-vs-float64 distance): stored in the
fixture, printed here.
"""
import os

import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.detach().cpu().contiguous().numpy()


def _rtol(g, key):
    return max(1e-4, 3.0 * float(g[key][0]))


def _make_block(tag):
    from spatiotemporalentropymodel_amd import layers as L
    return {"rbs_3_32": lambda: L.ResidualBlockWithStride(3, 32), "rbs_32_32": lambda: L.ResidualBlockWithStride(32, 32),
            "rb_32_32": lambda: L.ResidualBlock(32, 32), "rbu_32_32": lambda: L.ResidualBlockUpsample(32, 32, 2),
            "attn_32": lambda: L.AttentionBlock(32), "attn_24": lambda: L.AttentionBlock(24)}[tag]()


@pytest.mark.parametrize("tag", ["rbs_3_32", "rbs_32_32", "rb_32_32", "rbu_32_32", "attn_32", "attn_24"])
def test_block_output_and_gradients_match_float64(golden, tag):
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_, closed_form_input
    g = golden("cheng_blocks.npz")
    blk = closed_form_fill_(_make_block(tag)).to(DEV)
    cin = 3 if tag == "rbs_3_32" else int(tag.rsplit("_", 1)[1])
    x = closed_form_input(f"cheng:{tag}:x", (2, cin, 6, 10), 0.0 if cin == 3 else -1.0, 1.0).to(DEV).requires_grad_(True)
    out = blk(x)
    assert tuple(out.shape) == g[f"{tag}:out"].shape
    assert_close(host(out), g[f"{tag}:out"], rtol=_rtol(g, f"{tag}:ref32:out"), what=f"{tag} output", floor=0.1)
    with torch.no_grad():                                                   # the inference routes (conv + GDN in one kernel)
        assert_close(host(blk(x.detach())), g[f"{tag}:out"], rtol=_rtol(g, f"{tag}:ref32:out"), what=f"{tag} output under no_grad", floor=0.1)
    out.backward(closed_form_input(f"cheng:{tag}:g", tuple(out.shape), -1.0, 1.0).to(DEV))
    torch.cuda.synchronize()
    assert_close(host(x.grad), g[f"{tag}:dx"], rtol=_rtol(g, f"{tag}:ref32:dx"), what=f"{tag} input gradient", floor=0.1)
    params = dict(blk.named_parameters())
    assert sorted(params) == sorted(g[f"{tag}:params"])
    for name in g[f"{tag}:params"]:
        assert params[name].grad is not None, name
        assert_close(host(params[name].grad), g[f"{tag}:d:{name}"], rtol=_rtol(g, f"{tag}:ref32:d:{name}"), what=f"{tag} d{name}", floor=0.1)


_MODELS = {}


def _scale_like_the_generator(m, g):
    """make_golden_cheng.build: the last analysis convolution x gain, the synthesis convolutions x g_s_scale"""
    from spatiotemporalentropymodel_amd.layers import Conv2d
    (last,) = [c for c in m.g_a.children() if isinstance(c, Conv2d)]
    with torch.no_grad():
        last.weight.mul_(float(g["gain"][0]))
        last.bias.mul_(float(g["gain"][0]))
        for p in m.g_s.parameters():
            if p.dim() == 4:
                p.mul_(float(g["g_s_scale"][0]))


def _model(golden, tag):
    """Cheng2020Anchor(64) / Cheng2020Attention(64) as make_golden_cheng.build makes them, the reference's tables loaded as a
    checkpoint brings them; built once per session"""
    if tag not in _MODELS:
        from spatiotemporalentropymodel_amd.models import Cheng2020Anchor, Cheng2020Attention
        from spatiotemporalentropymodel_amd.weights import closed_form_fill_
        g = golden(f"cheng_codec.{tag}.npz")
        m = closed_form_fill_({"anchor": Cheng2020Anchor, "attn": Cheng2020Attention}[tag](int(g["N"][0])))
        _scale_like_the_generator(m, g)
        m = m.to(DEV).eval()
        assert m.update(force=True) is True
        sd = m.state_dict()
        for k in ("entropy_bottleneck._quantized_cdf", "entropy_bottleneck._offset", "entropy_bottleneck._cdf_length",
                  "gaussian_conditional._quantized_cdf", "gaussian_conditional._offset", "gaussian_conditional._cdf_length"):
            if k.endswith("_quantized_cdf"):
                diff = np.abs(host(sd[k]).astype(np.int64) - g[k])
                assert diff.max() <= 1 and (diff != 0).mean() < 5e-3, k
            sd[k] = torch.from_numpy(g[k]).to(DEV)
        m.load_state_dict(sd)
        _MODELS[tag] = (m, g)
    return _MODELS[tag]


def _image(g, i):
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    h, w = (int(v) for v in g["sizes"][i])
    return smooth_frames(str(g["seeds"][i]), 1, 1, max(h, w))[0][:, :, :h, :w].contiguous().to(DEV)


def _print_margins(g, i, tag):
    print(f"[{tag} image {i}: {g['seeds'][i]}, gain {float(g['gain'][0])}] margins (in units of the reference's fp32 distance): " +
          ", ".join(f"{n} {m:.2e} ({m / max(d, 1e-300):.0f} x)" for n, m, d in zip(g[f"{i}:margin_names"], g[f"{i}:margins"], g[f"{i}:margin_ref32"])))


@pytest.mark.parametrize("tag", ["anchor", "attn"])
@pytest.mark.parametrize("i", [0, 1])
def test_eval_forward_matches_float64(golden, tag, i):
    m, g = _model(golden, tag)
    with torch.no_grad():
        fwd = m(_image(g, i))
    ours = {"y": fwd["y"], "y_hat": fwd["y_hat"], "x_hat": fwd["x_hat"], "lik_y": fwd["likelihoods"]["y"], "lik_z": fwd["likelihoods"]["z"],
            "scales": fwd["entropy_params"]["scales_hat"], "means": fwd["entropy_params"]["means_hat"]}
    _print_margins(g, i, tag)
    for k, v in ours.items():
        assert_close(host(v), g[f"{i}:fwd:{k}"], rtol=_rtol(g, f"{i}:ref32:{k}"), atol=1e-9 if k.startswith("lik") else 0.0,
                     what=f"{tag} image {i}: forward {k}", floor=0.1)


def _first_difference(a, b):
    n = min(len(a), len(b))
    k = next((j for j in range(n) if a[j] != b[j]), n)
    return f"lengths {len(a)} / {len(b)}, first differing byte {k}"


@pytest.mark.parametrize("tag", ["anchor", "attn"])
@pytest.mark.parametrize("i", [0, 1])
def test_codec_matches_reference(golden, tag, i):
    """compress: both strings byte for byte.  decompress of the reference's strings on both decoder routes: y_hat equal to the
    reference's, x_hat within the gate, the two routes identical."""
    from spatiotemporalentropymodel_amd import config
    m, g = _model(golden, tag)
    x = _image(g, i)
    _print_margins(g, i, tag)
    ref_y, ref_z = g[f"{i}:y_string"].tobytes(), g[f"{i}:z_string"].tobytes()
    with torch.no_grad():
        enc = m.compress(x)
        assert tuple(enc["shape"]) == tuple(g[f"{i}:shape"])
        assert enc["strings"][1][0] == ref_z, "hyper-latent bitstream differs: " + _first_difference(enc["strings"][1][0], ref_z)
        assert enc["strings"][0][0] == ref_y, "latent bitstream differs from the reference's: " + _first_difference(enc["strings"][0][0], ref_y)
        outs = []
        for persistent in ("1", "0"):
            os.environ["STEM_AR_PERSISTENT"] = persistent
            try:
                assert config.runtime().ar_persistent == (persistent == "1")
                outs.append(m.decompress([[ref_y], [ref_z]], enc["shape"]))
            finally:
                os.environ.pop("STEM_AR_PERSISTENT")
    assert torch.equal(outs[0]["y_hat"], outs[1]["y_hat"]) and torch.equal(outs[0]["x_hat"], outs[1]["x_hat"])
    # y_hat = (decoded integer) + means_hat: equal symbols; the means carry fp32 noise
    assert_close(host(outs[0]["y_hat"]), g[f"{i}:y_hat"], rtol=_rtol(g, f"{i}:ref32:means"), what="decoded y_hat", floor=0.1)
    assert float(np.abs(host(outs[0]["y_hat"]) - g[f"{i}:y_hat"]).max()) < 0.25, "a decoded symbol differs"
    # the image is g_s's output clamped to [0, 1]: a pixel next to a clamp edge carries the UNclamped tensor's error
    pre = max(float(np.abs(g[f"{i}:fwd:x_hat"]).max()), 1.0)
    assert_close(host(outs[0]["x_hat"]), g[f"{i}:x_hat"], rtol=_rtol(g, f"{i}:ref32:x_hat"), atol=_rtol(g, f"{i}:ref32:x_hat") * pre,
                 what="decoded image", floor=0.1)


@pytest.mark.parametrize("tag", ["anchor", "attn"])
def test_wavefront_order_round_trip(golden, tag):
    m, g = _model(golden, tag)
    x = _image(g, 1)
    with torch.no_grad():
        raster = m.compress(x)
        wave = m.compress(x, order="wavefront")
        assert wave["strings"][1] == raster["strings"][1]
        a = m.decompress(raster["strings"], raster["shape"])
        b = m.decompress(wave["strings"], wave["shape"], order="wavefront")
    assert torch.equal(a["y_hat"], b["y_hat"]) and torch.equal(a["x_hat"], b["x_hat"])


@pytest.mark.parametrize("tag", ["anchor", "attn"])
def test_compress_each_gives_the_bytes_of_each_alone(golden, tag):
    from spatiotemporalentropymodel_amd import codec
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    m, g = _model(golden, tag)
    xs = [_image(g, 0), smooth_frames("cheng:each", 1, 1, 128)[0].to(DEV)]
    with torch.no_grad():
        both = codec.iframe_compress_each(m, xs)
        for x, res in zip(xs, both):
            alone = m.compress(x)
            assert res["strings"] == alone["strings"] and tuple(res["shape"]) == tuple(alone["shape"])
        dec = codec.iframe_decompress_each(m, [r["strings"] for r in both], [r["shape"] for r in both])
        for res, d in zip(both, dec):
            assert torch.equal(d["y_hat"], m.decompress(res["strings"], res["shape"])["y_hat"])


@pytest.mark.parametrize("persistent", ["1", "0"])
def test_eval_gop_with_a_cheng_iframe_model(golden, persistent, monkeypatch):
    """evaluation.eval_gop(Cheng2020Anchor(96), SpatioTemporalPriorModel_Res(64, 96), ...) against the reference's own
    inferenceI_DVR / inferenceP_DVR on the same frames: strings byte for byte, bpp equal, rate estimate and PSNR within 1e-4"""
    from spatiotemporalentropymodel_amd import config, evaluation
    from spatiotemporalentropymodel_amd.models import Cheng2020Anchor, SpatioTemporalPriorModel_Res
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_, smooth_frames
    g = golden("cheng_gop.npz")
    imodel = closed_form_fill_(Cheng2020Anchor(int(g["N"][0])))
    _scale_like_the_generator(imodel, g)
    stem = closed_form_fill_(SpatioTemporalPriorModel_Res(64, 96))
    models = []
    for tag, m in (("i", imodel), ("p", stem)):
        m = m.to(DEV).eval()
        assert m.update(force=True) is True
        sd = m.state_dict()
        for k, v in (("entropy_bottleneck._quantized_cdf", g[f"{tag}:eb_cdf"]), ("entropy_bottleneck._offset", g[f"{tag}:eb_offset"]),
                     ("entropy_bottleneck._cdf_length", g[f"{tag}:eb_cdf_length"]), ("gaussian_conditional._quantized_cdf", g[f"{tag}:gc_cdf"]),
                     ("gaussian_conditional._offset", g[f"{tag}:gc_offset"]), ("gaussian_conditional._cdf_length", g[f"{tag}:gc_cdf_length"])):
            sd[k] = torch.from_numpy(v).to(DEV)
        m.load_state_dict(sd)
        models.append(m)
    h, w = (int(v) for v in g["size"])
    n = int(g["nframes"][0])
    frames = [f[0, :, 4:4 + h, 12:12 + w].contiguous().to(DEV) for f in smooth_frames("cheng:gop", 1, n, 128)]
    monkeypatch.setenv("STEM_AR_PERSISTENT", persistent)
    assert config.runtime().ar_persistent == (persistent == "1")
    res = evaluation.eval_gop(models[0], models[1], frames, gop=12)
    assert [f["type"] for f in res["frames"]] == ["I"] + ["P"] * (n - 1)
    for t, f in enumerate(res["frames"]):
        assert tuple(f["shape"]) == tuple(g[f"f{t}:shape"])
        assert f["strings"][1][0] == g[f"f{t}:z_string"].tobytes(), f"frame {t}: hyper-latent bitstream differs"
        assert f["strings"][0][0] == g[f"f{t}:y_string"].tobytes(), f"frame {t}: latent bitstream differs from the reference's"
        bpp, est, ps = g[f"f{t}:scalars"]
        assert f["bpp"] == bpp
        assert abs(f["estimate_bpp"] - est) <= 1e-4 * abs(est), (t, f["estimate_bpp"], est)
        assert abs(f["psnr"] - ps) <= 1e-4 * abs(ps), (t, f["psnr"], ps)
        assert_close(host(f["y_conditioned"]), g[f"f{t}:y_conditioned"], what=f"frame {t}: decoded latents", floor=0.1)
    assert_close(host(res["frames"][-1]["x_hat"]), g["last:x_hat"], atol=1e-4, what="last frame's reconstruction", floor=0.1)
