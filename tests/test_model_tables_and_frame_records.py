"""CPU: what CompressionModel states once for every model -- update() / load_state_dict of the bottleneck's and the Gaussian tables --
and what evaluation.py states once for every loop: the per-frame dictionary (`_frame_record`) and the sequence averages
(`_sequence_averages`), on hand-made coder outputs.  No device."""
import math

import pytest
import torch

GC_BUFFERS = ("_quantized_cdf", "_offset", "_cdf_length", "scale_table")


def _make(name):
    from spatiotemporalentropymodel_amd import models
    return {"mbt2018": lambda: models.JointAutoregressiveHierarchicalPriors(16, 24), "mbt2018-mean": lambda: models.MeanScaleHyperprior(16, 24),
            "hyperprior": lambda: models.ScaleHyperprior(16, 24), "stem": lambda: models.SpatioTemporalPriorModel(16, 24),
            "pixel": lambda: models.stem_baseline(256, 24)}[name]()


@pytest.mark.parametrize("name", ["mbt2018", "mbt2018-mean", "hyperprior", "stem", "pixel"])
def test_update_and_load_state_dict_handle_the_gaussian_tables(name):
    from spatiotemporalentropymodel_amd.models.priors import CompressionModel, get_scale_table
    src = _make(name)
    for owner in type(src).__mro__:                     # the one statement is the base class's
        if "update" in vars(owner) or "load_state_dict" in vars(owner):
            assert owner is CompressionModel or owner is torch.nn.Module, owner
    gc = src.gaussian_conditional
    assert all(getattr(gc, b).numel() == 0 for b in GC_BUFFERS) and src.entropy_bottleneck._offset.numel() == 0
    assert src.update(force=True) is True and src.update() is False
    assert torch.equal(gc.scale_table, get_scale_table()) and gc._quantized_cdf.shape[0] == 64 and gc._quantized_cdf.dim() == 2
    assert gc._offset.numel() == gc._cdf_length.numel() == 64 and src.entropy_bottleneck._quantized_cdf.dim() == 2
    assert src.update(scale_table=get_scale_table(levels=8), force=True) is True and gc._offset.numel() == gc.scale_table.numel() == 8
    dst = _make(name)                                   # fresh: empty table buffers
    dst.load_state_dict(src.state_dict())
    for b in GC_BUFFERS:
        assert getattr(dst.gaussian_conditional, b).shape == getattr(gc, b).shape and torch.equal(getattr(dst.gaussian_conditional, b), getattr(gc, b)), b
    for (k, a), (k2, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert k == k2 and a.shape == b.shape and torch.equal(a, b), k
    assert dst.update() is False                        # the tables came with the checkpoint


def test_factorized_prior_updates_without_gaussian_tables():
    from spatiotemporalentropymodel_amd.models import FactorizedPrior
    m = FactorizedPrior(16, 24)
    assert not hasattr(m, "gaussian_conditional")
    assert m.update() is True and m.update() is False and m.update(force=True) is True and m.update(None, True) is True
    assert m.entropy_bottleneck._quantized_cdf.dim() == 2 and m.entropy_bottleneck._offset.numel() == 24
    dst = FactorizedPrior(16, 24)
    dst.load_state_dict(m.state_dict())
    assert torch.equal(dst.entropy_bottleneck._quantized_cdf, m.entropy_bottleneck._quantized_cdf) and dst.update() is False


def test_get_scale_table_has_one_home():
    from spatiotemporalentropymodel_amd.models import priors, spatiotemporalpriors
    assert spatiotemporalpriors.get_scale_table is priors.get_scale_table and "get_scale_table" in spatiotemporalpriors.__all__
    t = priors.get_scale_table()
    assert t.shape == (64,) and abs(float(t[0]) - 0.11) < 1e-6 and abs(float(t[-1]) - 256) < 1e-3


# ----------------------------------------------------------------------------- evaluation.py
SHARED = {"psnr", "ms-ssim", "bpp", "estimate_bpp", "estimate_y_bpp", "estimate_z_bpp", "y_bpp", "z_bpp", "encoding_time", "decoding_time",
          "strings", "shape", "x_hat"}
H, W = 4, 6


def _coder_outputs(n_strings):
    """a frame [1,3,4,6], its reconstruction, and what compress / forward would have returned: strings of 3 and 2 bytes, likelihoods 1/2 and 1/4"""
    x = torch.full((1, 3, H, W), 0.5)
    x_hat = x + 0.1
    strings = [[b"abc"], [b"de"]][:n_strings]
    lik = {"y": torch.full((1, 2, 2, 3), 0.5), "z": torch.full((1, 2, 1, 1), 0.25)}
    if n_strings == 1:
        del lik["z"]
    return x, x_hat, {"strings": strings, "shape": torch.Size([1, 2])}, {"likelihoods": lik}


@pytest.mark.parametrize("n_strings", [1, 2])
def test_frame_record_keys_and_values(n_strings):
    from spatiotemporalentropymodel_amd import evaluation
    x, x_hat, out_enc, out_forward = _coder_outputs(n_strings)
    rec = evaluation._frame_record(x, x_hat, out_enc, out_forward, (0.25, 0.5), False)
    assert set(rec) == SHARED
    px = H * W
    assert rec["y_bpp"] == 3 * 8.0 / px and rec["bpp"] == (3 + 2 * (n_strings - 1)) * 8.0 / px
    if n_strings == 1:
        assert rec["z_bpp"] is None and rec["estimate_z_bpp"] is None
        assert abs(rec["estimate_bpp"] - 12 / px) < 1e-6
    else:
        assert rec["z_bpp"] == 2 * 8.0 / px and abs(rec["estimate_z_bpp"] - 4 / px) < 1e-6
        assert abs(rec["estimate_bpp"] - 16 / px) < 1e-6
    assert abs(rec["estimate_y_bpp"] - 12 / px) < 1e-6                          # 12 latents at one bit each
    assert abs(rec["psnr"] - 20.0) < 1e-4 and rec["ms-ssim"] is None            # error 0.1 everywhere
    assert (rec["encoding_time"], rec["decoding_time"]) == (0.25, 0.5)
    assert rec["strings"] is out_enc["strings"] and rec["shape"] == (1, 2) and type(rec["shape"]) is tuple and rec["x_hat"] is x_hat
    # the key sets of the public callers: inference_iframe, inference_pframe, eval_sequence's I and P frames, inference_pixel_i / _p
    yuv = {"psnr_y": 1.0, "psnr_u": 2.0, "psnr_v": 3.0, "psnr_yuv": 1.5}
    for own in ({"y_conditioned": 0, "out_forward": out_forward}, {"y_conditioned": 0, "entropy_params": None},
                {"y_conditioned": 0, "out_forward": out_forward, "type": "I", "concurrent": 3}, {"y_conditioned": 0, "entropy_params": None, "type": "P", "concurrent": 3},
                {"y_conditioned": 0, "out_forward": out_forward, **yuv}, {"bits": 40.0}):
        rec = evaluation._frame_record(x, x_hat, out_enc, out_forward, (0.25, 0.5), False, **own)
        assert set(rec) == SHARED | set(own) and all(rec[k] is v for k, v in own.items())
        assert (rec["z_bpp"] is None) == (n_strings == 1)


def test_sequence_averages_keys_and_values():
    from spatiotemporalentropymodel_amd import evaluation
    frames = [{"psnr": 30.0, "ms-ssim": None, "bpp": 1.0, "estimate_bpp": 0.5, "bits": 8.0, "psnr_roi": float("inf"), "psnr_y": 1.0, "psnr_u": 2.0,
               "psnr_v": 3.0, "psnr_yuv": 1.5},
              {"psnr": 34.0, "ms-ssim": 0.75, "bpp": 2.0, "estimate_bpp": 1.5, "bits": 24.0, "psnr_roi": 31.0, "psnr_y": 3.0, "psnr_u": 4.0,
               "psnr_v": 5.0, "psnr_yuv": 3.5},
              {"psnr": 35.0, "ms-ssim": 0.25, "bpp": 3.0, "estimate_bpp": 1.0, "bits": 40.0, "psnr_y": 5.0, "psnr_u": 6.0, "psnr_v": 7.0, "psnr_yuv": 5.5}]
    base = {"frames", "psnr_ave", "bpp_ave", "msssim_ave", "estimate_bpp_ave"}
    res = evaluation._sequence_averages(frames)                                  # eval_gop / eval_sequence
    assert set(res) == base and res["frames"] is frames
    assert (res["psnr_ave"], res["bpp_ave"], res["msssim_ave"], res["estimate_bpp_ave"]) == (33.0, 2.0, 0.5, 1.0)
    res = evaluation._sequence_averages(frames, evaluation._YUV_KEYS)            # ... with yuv=True
    assert set(res) == base | {"psnr_y_ave", "psnr_u_ave", "psnr_v_ave", "psnr_yuv_ave"}
    assert (res["psnr_y_ave"], res["psnr_u_ave"], res["psnr_v_ave"], res["psnr_yuv_ave"]) == (3.0, 4.0, 5.0, 3.5)
    res = evaluation._sequence_averages(frames, ("bits",), psnr_roi=True)        # eval_gop_pixel
    assert set(res) == base | {"bits_ave", "psnr_roi_ave"} and res["bits_ave"] == 24.0
    assert res["psnr_roi_ave"] == 31.0                                           # the finite ones only
    none = evaluation._sequence_averages([dict(frames[0])], ("bits",), psnr_roi=True)
    assert none["psnr_roi_ave"] is None and none["msssim_ave"] is None and none["psnr_ave"] == 30.0
    empty = evaluation._sequence_averages([])
    assert empty["frames"] == [] and empty["psnr_ave"] == 0 and empty["msssim_ave"] is None and not math.isnan(empty["bpp_ave"])
