"""What tests/golden/make_golden_pixel_eval.py fed to the reference, restated for the tests of the pixel-domain evaluation loop: the
three 104 x 72 frames and the models on their closed-form weights, with the CDF tables the reference built."""
import numpy as np
import torch

SIZE = (104, 72)
TOP, LEFT = 12, 28
ROI_CONV_SCALE = 0.7


def frames3():
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    h, w = SIZE
    return [f[0, :, TOP:TOP + h, LEFT:LEFT + w].contiguous() for f in smooth_frames("pixeleval", 1, 3, 128)]


def build(cls, tag, scale, dev, g=None, *args):
    """cls(*args) on closed_form_fill_scaled_(tag, scale) in eval mode with its tables; g: a fixture holding the reference's tables of
    `tag` -- the bottleneck's are installed (they pass through libm), the Gaussians' must equal ours entry for entry"""
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_scaled_
    m = closed_form_fill_scaled_(cls(*args), tag, scale).to(dev).eval()
    m.update(force=True)
    if g is not None:
        for k in ("_quantized_cdf", "_offset", "_cdf_length"):
            getattr(m.entropy_bottleneck, k).copy_(torch.from_numpy(g[f"{tag}:entropy_bottleneck.{k}"]))
            np.testing.assert_array_equal(getattr(m.gaussian_conditional, k).cpu().numpy(), g[f"{tag}:gaussian_conditional.{k}"])
    return m


def roi_chain(dev, g):
    from spatiotemporalentropymodel_amd.models import stem_roi, stem_roi_i
    return build(stem_roi_i, "roi_i", ROI_CONV_SCALE, dev, g), build(stem_roi, "roi_p", ROI_CONV_SCALE, dev, g)


def baseline_chain(dev, g):
    from spatiotemporalentropymodel_amd.models import MeanScaleHyperprior, stem_baseline
    return build(MeanScaleHyperprior, "msh", 1.0, dev, g, 64, 96), build(stem_baseline, "base_p", ROI_CONV_SCALE, dev, g)
