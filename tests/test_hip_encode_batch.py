"""GPU: the batched raster-order encoder (csrc/ar.hip: stem_ar_encode_batch) against stem_ar_encode_image image by image, the
batched codec._encode_latents and the per-chain entry points of codec.py against the single-image functions, and
evaluation.eval_sequence (a sequence's GOPs coded side by side) against evaluation.eval_gop: bit for bit at every level."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(cls_name, widths):
    """closed-form weights as in test_hip_codec.py; one instance per geometry for the whole module"""
    import spatiotemporalentropymodel_amd.models as M
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    key = (cls_name, widths)
    if key not in _MODELS:
        m = closed_form_fill_(getattr(M, cls_name)(*widths)).to(torch.device("cuda:0")).eval()
        m.update(force=True)
        _MODELS[key] = m
    return _MODELS[key]


def _nhwc(tag, shape, lo, hi):
    from spatiotemporalentropymodel_amd import codec, functional as F
    from spatiotemporalentropymodel_amd.weights import closed_form_input
    return codec._dense(F.to_nhwc(closed_form_input(tag, shape, lo, hi).to(torch.device("cuda:0"))))


def _latents(m, M, G, H, W, tag):
    """(target, hp, tp): dense NHWC latents and priors of G images; tp is None for a model without temporal prior"""
    target = _nhwc(f"{tag}:y", (G, M, H, W), -6.0, 6.0)
    hp = _nhwc(f"{tag}:hp", (G, 2 * M, H, W), -1.0, 1.0)
    tp = _nhwc(f"{tag}:tp", (G, 2 * M, H, W), -1.0, 1.0) if m.HAS_TPM else None
    return target, hp, tp


# H x W / G of the issue, plus 26 x 80 / 5: G * np = 130 positions in a step, more than WAVE_U = 4 times the WAVE_ROWS_B = 32 workgroup
# rows, so a wavefront takes four positions side by side, then a single one (26 x 80 / 2: two side by side, then one)
SHAPES = [(8, 12, 1), (8, 12, 5), (12, 4, 3), (1, 2, 2), (4, 12, 9), (26, 80, 2), (26, 80, 5)]
CASES = ([("SpatioTemporalPriorModel_Res", (64, 96), s) for s in SHAPES] + [("SpatioTemporalPriorModelWithoutTPM", (64, 96), s) for s in SHAPES[:-1]]
         + [("SpatioTemporalPriorModel_Res", (256, 192), (8, 12, 5))])


@pytest.mark.parametrize("cls_name,widths,shape", CASES)
def test_encode_batch_equals_encode_image(cls_name, widths, shape):
    """sym, idx and the returned buf of one stem_ar_encode_batch call against G stem_ar_encode_image calls on the same inputs"""
    from spatiotemporalentropymodel_amd import codec
    H, W, G = shape
    M = widths[1]
    m = _model(cls_name, widths)
    dev = torch.device("cuda:0")
    ar = codec._ARContext(m, dev)
    target, hp, tp = _latents(m, M, G, H, W, f"eb:{H}x{W}x{G}")
    buf = torch.zeros((G, H + 4, W + 4, M), device=dev)
    buf[:, 2:2 + H, 2:2 + W].permute(0, 3, 1, 2).copy_(target)
    ref_buf = buf.clone()
    sym, idx = (torch.full((G, H * W, M), -12345, device=dev, dtype=torch.int32) for _ in range(2))
    ar.encode_batch(buf, G, H, W, *codec._prior_addrs(tp, hp, 0, H, W, M), sym, idx)
    ref_sym, ref_idx = (torch.full((G, H * W, M), -54321, device=dev, dtype=torch.int32) for _ in range(2))
    for g in range(G):
        ar.encode_wavefront(ref_buf[g], H, W, *codec._prior_addrs(tp, hp, g, H, W, M), ref_sym[g], ref_idx[g])     # stem_ar_encode_image
    torch.cuda.synchronize()
    assert torch.equal(sym, ref_sym), "symbols differ"
    assert torch.equal(idx, ref_idx), "indexes differ"
    assert torch.equal(buf, ref_buf), "reconstruction (or the zero border) differs"
    assert int(idx.min()) >= 0 and int(sym.abs().max()) > 0 and not torch.equal(buf[:, 2:2 + H, 2:2 + W].permute(0, 3, 1, 2), target)


def test_encode_batch_refuses_bad_arguments():
    from spatiotemporalentropymodel_amd import _lib, codec, functional as F
    H, W, G, M = 4, 6, 2, 96
    m = _model("SpatioTemporalPriorModel_Res", (64, 96))
    dev = torch.device("cuda:0")
    ar = codec._ARContext(m, dev)
    lib = _lib.hip()
    _, hp, tp = _latents(m, M, G, H, W, "eb:bad")
    buf = torch.zeros((G, H + 4, W + 4, M), device=dev)
    sym, idx = (torch.zeros((G, H * W, M), device=dev, dtype=torch.int32) for _ in range(2))
    scratch = [torch.empty((G, 2, n), device=dev) for n in (2 * M, ar.w0.shape[0], ar.w1.shape[0], 2 * M)]

    def call(G=G, hp_ptr=hp.data_ptr(), pad=2):
        rc = lib.stem_ar_encode_batch(*ar.net_args(), buf.data_ptr(), G, H, W, M, pad, tp.data_ptr(), hp_ptr, *[t.data_ptr() for t in scratch],
                                      *ar.table_args(), sym.data_ptr(), idx.data_ptr(), F._stream())
        return rc, lib.stem_last_error() or b""

    for kw in (dict(G=0), dict(hp_ptr=None), dict(pad=1), dict(pad=3)):
        rc, msg = call(**kw)
        assert rc != 0 and b"stem_ar_encode_batch" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert int(sym.abs().max()) == 0 and float(buf.abs().max()) == 0.0          # nothing ran
    assert call()[0] == 0
    torch.cuda.synchronize()


def test_encode_latents_of_a_batch_equals_the_per_image_loop():
    """codec._encode_latents on B = 5 (one stem_ar_encode_batch call, one copy, the host coder on the pool) gives the bytes of five
    B = 1 calls (stem_ar_encode_image) on the slices of the same hp / tp"""
    from spatiotemporalentropymodel_amd import codec
    for cls_name in ("SpatioTemporalPriorModel_Res", "SpatioTemporalPriorModelWithoutTPM"):
        m = _model(cls_name, (64, 96))
        target, hp, tp = _latents(m, 96, 5, 8, 12, "el")
        with torch.no_grad():
            batch = codec._encode_latents(m, target, hp, tp)
            alone = [codec._encode_latents(m, target[b:b + 1], hp[b:b + 1], None if tp is None else tp[b:b + 1])[0] for b in range(5)]
        assert len(batch) == 5 and all(isinstance(s, bytes) and len(s) > 8 for s in batch)
        assert batch == alone
        assert len(set(batch)) == 5


def test_stem_each_equals_the_single_chain_functions():
    """stem_compress_each -> stem_decompress_each over 3 chains: per chain the strings (byte for byte) and y_hat (torch.equal) of
    stem_compress / stem_decompress of that chain alone at batch 1"""
    from spatiotemporalentropymodel_amd import codec
    from spatiotemporalentropymodel_amd.weights import closed_form_input
    dev = torch.device("cuda:0")
    for cls_name in ("SpatioTemporalPriorModel_Res", "SpatioTemporalPriorModelWithoutTPM"):
        m = _model(cls_name, (64, 96))
        y_cur = closed_form_input("se:y", (3, 96, 8, 12), -6, 6).to(dev)
        y_cond = closed_form_input("se:c", (3, 96, 8, 12), -6, 6).to(dev)
        curs, conds = [y_cur[i:i + 1] for i in range(3)], [y_cond[i:i + 1] for i in range(3)]
        with torch.no_grad():
            encs = codec.stem_compress_each(m, curs, conds)
            decs = codec.stem_decompress_each(m, [e["strings"] for e in encs], [e["shape"] for e in encs], conds)
            for i in range(3):
                enc = codec.stem_compress(m, curs[i], conds[i])
                assert set(encs[i]) == set(enc) and tuple(encs[i]["shape"]) == tuple(enc["shape"])
                assert encs[i]["strings"] == enc["strings"], f"{cls_name}: chain {i}: strings differ"
                y_hat = codec.stem_decompress(m, enc["strings"], enc["shape"], conds[i])
                assert decs[i].shape == y_hat.shape and torch.equal(decs[i], y_hat), f"{cls_name}: chain {i}: y_hat differs"
                assert float((decs[i] - curs[i]).abs().max()) <= 0.5 + 1e-4
        assert len({e["strings"][0][0] for e in encs}) == 3
        with pytest.raises(ValueError):
            codec.stem_compress_each(m, [y_cur[0:2]], [y_cond[0:2]])                 # one [1, ...] tensor per chain


@pytest.fixture(scope="module")
def gop_models(golden):
    from test_hip_codec import _eval_gop_models
    return _eval_gop_models(golden("eval_gop.npz"), torch.device("cuda:0"))


@pytest.fixture(scope="module")
def golden_frames(golden):
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    g = golden("eval_gop.npz")
    h, w = (int(v) for v in g["size"])
    n = int(g["nframes"][0])
    return [f[0, :, 4:4 + h, 12:12 + w].contiguous().to(torch.device("cuda:0")) for f in smooth_frames("evalgop", 1, n, 128)]


def test_iframe_each_equals_the_single_image_functions(gop_models, golden_frames):
    from spatiotemporalentropymodel_amd import bitstream, codec
    imodel, _ = gop_models
    xs = [bitstream.pad(f.unsqueeze(0), 64) for f in golden_frames]
    with torch.no_grad():
        encs = codec.iframe_compress_each(imodel, xs)
        decs = codec.iframe_decompress_each(imodel, [e["strings"] for e in encs], [e["shape"] for e in encs])
        for i, x in enumerate(xs):
            enc = codec.iframe_compress(imodel, x)
            assert set(encs[i]) == set(enc) and tuple(encs[i]["shape"]) == tuple(enc["shape"])
            assert encs[i]["strings"] == enc["strings"], f"image {i}: strings differ"
            dec = codec.iframe_decompress(imodel, enc["strings"], enc["shape"])
            assert set(decs[i]) == set(dec)
            assert torch.equal(decs[i]["y_hat"], dec["y_hat"]) and torch.equal(decs[i]["x_hat"], dec["x_hat"]), f"image {i}: decoded image differs"


def _sequence(golden_frames):
    """7 frames: the golden frames, their horizontal flips, and the first one again -- gop 2: I P | I P | I P | I"""
    return golden_frames + [f.flip(-1).contiguous() for f in golden_frames] + golden_frames[:1]


@pytest.fixture(scope="module")
def gop_runs(gop_models, golden_frames, tmp_path_factory):
    """eval_gop(gop=2) of the 7-frame sequence, plain and with yuv=True / write_to: the reference of the eval_sequence tests"""
    from spatiotemporalentropymodel_amd import evaluation
    imodel, stem = gop_models
    frames = _sequence(golden_frames)
    path = tmp_path_factory.mktemp("seq") / "eval_gop.yuv"
    return {"frames": frames, "plain": evaluation.eval_gop(imodel, stem, frames, gop=2),
            "yuv": evaluation.eval_gop(imodel, stem, frames, gop=2, yuv=True, write_to=path), "bytes": path.read_bytes()}


def _same_frames(got, want, extra=()):
    assert len(got["frames"]) == len(want["frames"])
    assert [f["type"] for f in got["frames"]] == [f["type"] for f in want["frames"]]
    for t, (a, b) in enumerate(zip(got["frames"], want["frames"])):
        assert set(b) | {"concurrent"} == set(a), (t, set(a) ^ set(b))
        assert a["strings"] == b["strings"], f"frame {t}: strings differ"
        assert tuple(a["shape"]) == tuple(b["shape"])
        for k in ("bpp", "estimate_bpp", "psnr", "y_bpp", "z_bpp", "estimate_y_bpp", "estimate_z_bpp", "ms-ssim") + tuple(extra):
            assert a[k] == b[k], (t, k, a[k], b[k])
        assert torch.equal(a["x_hat"], b["x_hat"]), f"frame {t}: x_hat differs"
        assert torch.equal(a["y_conditioned"], b["y_conditioned"]), f"frame {t}: y_conditioned differs"
    for k in want:
        if k != "frames":
            assert got[k] == want[k], (k, got[k], want[k])
    assert set(got) == set(want)


def test_eval_sequence_equals_eval_gop(gop_models, gop_runs):
    """gop 2, three GOPs side by side: groups of 3 and 1 GOPs, the last GOP one frame long"""
    from spatiotemporalentropymodel_amd import evaluation
    imodel, stem = gop_models
    res = evaluation.eval_sequence(imodel, stem, gop_runs["frames"], gop=2, concurrent_gops=3)
    assert [f["type"] for f in res["frames"]] == ["I", "P", "I", "P", "I", "P", "I"]
    assert [f["concurrent"] for f in res["frames"]] == [3, 3, 3, 3, 3, 3, 1]
    _same_frames(res, gop_runs["plain"])
    assert all(f["encoding_time"] > 0 and f["decoding_time"] > 0 for f in res["frames"])


def test_eval_sequence_writes_frames_in_display_order(gop_models, gop_runs, tmp_path):
    from spatiotemporalentropymodel_amd import evaluation
    imodel, stem = gop_models
    path = tmp_path / "eval_sequence.yuv"
    res = evaluation.eval_sequence(imodel, stem, gop_runs["frames"], gop=2, concurrent_gops=3, yuv=True, write_to=path)
    assert path.read_bytes() == gop_runs["bytes"]
    for k in ("psnr_y_ave", "psnr_u_ave", "psnr_v_ave", "psnr_yuv_ave"):
        assert res[k] == gop_runs["yuv"][k], k
    _same_frames(res, gop_runs["yuv"], extra=("psnr_y", "psnr_u", "psnr_v", "psnr_yuv"))


def test_eval_sequence_with_one_chain_per_step_equals_eval_gop(gop_models, gop_runs):
    from spatiotemporalentropymodel_amd import evaluation
    imodel, stem = gop_models
    res = evaluation.eval_sequence(imodel, stem, iter(gop_runs["frames"]), gop=2, concurrent_gops=1)
    assert [f["concurrent"] for f in res["frames"]] == [1] * 7
    _same_frames(res, gop_runs["plain"])


def test_eval_sequence_reproduces_the_reference_strings(golden, gop_models, golden_frames):
    """one chain (gop 12, three frames) against the reference's own bytes: tests/golden/eval_gop.npz"""
    from spatiotemporalentropymodel_amd import evaluation
    g = golden("eval_gop.npz")
    imodel, stem = gop_models
    res = evaluation.eval_sequence(imodel, stem, golden_frames, gop=12, concurrent_gops=8)
    assert [f["type"] for f in res["frames"]] == ["I"] + ["P"] * (len(golden_frames) - 1)
    for t, f in enumerate(res["frames"]):
        assert tuple(f["shape"]) == tuple(g[f"f{t}:shape"])
        assert f["strings"][1][0] == g[f"f{t}:z_string"].tobytes(), f"frame {t}: hyper-latent bitstream differs"
        assert f["strings"][0][0] == g[f"f{t}:y_string"].tobytes(), f"frame {t}: latent bitstream differs from the reference's"
        assert f["bpp"] == g[f"f{t}:scalars"][0]
    assert abs(res["bpp_ave"] - np.mean([g[f"f{t}:scalars"][0] for t in range(len(golden_frames))])) < 1e-12
