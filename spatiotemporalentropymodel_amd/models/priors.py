"""CompressionModel base class, the I-frame transforms of JointAutoregressiveHierarchicalPriors
("mbt2018": compressai/models/priors.py:42-106, 406-694), MeanScaleHyperprior ("mbt2018-mean": priors.py:196-402), the I-frame
model stem_roi/eval_stem_baseline.py pairs with stem_baseline, and its two zero-mean relatives FactorizedPrior ("bmshj2018-factorized":
priors.py:109-181) and ScaleHyperprior ("bmshj2018-hyperprior": priors.py:196-313).

On the STEM training path only g_a / g_s (getY / getX) are executed.  The evaluation loop also codes its I frames with this
model (stem/evalSTEM.py:54-59: compress / decompress; priors.py:476-716): forward (inference), compress and decompress run the
hyper-prior modules and the same raster-order coder as the STEM models (codec.py: the entropy-parameter network sees
cat(params, ctx) exactly like a STEM model without temporal prior).
"""
import torch
import torch.nn as nn

from .. import functional as F
from ..entropy_models import EntropyBottleneck, GaussianConditional
from ..layers import GDN, AbsFunction, Conv2d, ConvTranspose2d, FusedSequential, LeakyReLU, MaskedConv2d, cat, conv, deconv
from .utils import update_registered_buffers

__all__ = ["CompressionModel", "JointAutoregressiveHierarchicalPriors", "MeanScaleHyperprior", "FactorizedPrior", "ScaleHyperprior"]


class CompressionModel(nn.Module):
    def __init__(self, entropy_bottleneck_channels, init_weights=True):
        super().__init__()
        self.entropy_bottleneck = EntropyBottleneck(entropy_bottleneck_channels)
        if init_weights:
            # As in the reference this runs BEFORE subclasses create their layers (priors.py:51-56), so
            # convolutions keep torch's default nn.Conv2d initialisation; kept for behavioural parity.
            self._initialize_weights()

    def aux_loss(self):
        return sum(m.loss() for m in self.modules() if isinstance(m, EntropyBottleneck))

    def _initialize_weights(self):
        """kaiming_normal_ weights, zero biases for every (transposed) convolution present (priors.py:67-72)."""
        for m in self.modules():
            if isinstance(m, (Conv2d, ConvTranspose2d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, *args):
        raise NotImplementedError()

    def update(self, force=False):
        updated = False
        for m in self.children():
            if not isinstance(m, EntropyBottleneck):
                continue
            updated |= m.update(force=force)
        return updated

    def load_state_dict(self, state_dict, strict=True):
        update_registered_buffers(self.entropy_bottleneck, "entropy_bottleneck",
                                  ["_quantized_cdf", "_offset", "_cdf_length"], state_dict)
        return super().load_state_dict(state_dict, strict=strict)


class JointAutoregressiveHierarchicalPriors(CompressionModel):
    def __init__(self, N=192, M=192, **kwargs):
        super().__init__(entropy_bottleneck_channels=N, **kwargs)
        self.g_a = FusedSequential(conv(3, N), GDN(N), conv(N, N), GDN(N), conv(N, N), GDN(N), conv(N, M))
        self.g_s = FusedSequential(deconv(M, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True),
                                   deconv(N, N), GDN(N, inverse=True), deconv(N, 3))
        self.h_a = FusedSequential(conv(M, N, stride=1, kernel_size=3), LeakyReLU(inplace=True),
                                   conv(N, N, stride=2, kernel_size=5), LeakyReLU(inplace=True),
                                   conv(N, N, stride=2, kernel_size=5))
        self.h_s = FusedSequential(deconv(N, M, stride=2, kernel_size=5), LeakyReLU(inplace=True),
                                   deconv(M, M * 3 // 2, stride=2, kernel_size=5), LeakyReLU(inplace=True),
                                   conv(M * 3 // 2, M * 2, stride=1, kernel_size=3))
        self.entropy_parameters = FusedSequential(Conv2d(M * 12 // 3, M * 10 // 3, 1), LeakyReLU(inplace=True),
                                                  Conv2d(M * 10 // 3, M * 8 // 3, 1), LeakyReLU(inplace=True),
                                                  Conv2d(M * 8 // 3, M * 6 // 3, 1))
        self.context_prediction = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)
        self.gaussian_conditional = GaussianConditional(None)
        self.N, self.M = int(N), int(M)

    # ---- the two entry points the STEM scripts use (priors.py:686-694, 397-402) ---------------
    def getY(self, x):
        """-> (y, y + U(-1/2,1/2)); the mbt2018 variant adds noise in eval mode too (priors.py:691)."""
        y = self.g_a(x)
        y_quantized = self.gaussian_conditional.quantize(y, "noise")
        return y, y_quantized

    def getX(self, y_hat):
        """g_s + clamp(0,1); returns a contiguous NCHW image batch (layout change and clamp fused)."""
        return F.to_nchw(self.g_s(y_hat), clamp01=True)

    # ---- the I-frame codec (priors.py:476-716; stem/evalSTEM.py:54-59) ---------------------------------------------------------
    #: what codec.py's raster-order coder asks a model: a spatial prior, no temporal prior, the latents themselves are coded
    HAS_SPM, HAS_TPM, RESIDUAL = True, False, False

    @property
    def in_channels(self):
        return self.M

    @property
    def EPM(self):
        return self.entropy_parameters

    def forward(self, x):
        """priors.py:476-508 -> {"y", "y_hat", "x_hat", "likelihoods": {"y", "z"}, "entropy_params": {"scales_hat", "means_hat"}}"""
        y = self.g_a(x)
        z = self.h_a(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        params = self.h_s(z_hat)
        y_hat = self.gaussian_conditional.quantize(y, "noise" if self.training else "dequantize")
        ctx_params = self.context_prediction(y_hat)
        gaussian_params = self.entropy_parameters(cat([params, ctx_params]))
        scales_hat, means_hat = gaussian_params.chunk(2, 1)
        _, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        x_hat = self.g_s(y_hat)
        return {"y": y, "y_hat": y_hat, "x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods},
                "entropy_params": {"scales_hat": scales_hat, "means_hat": means_hat}}

    def compress(self, x, order="raster"):
        """priors.py:544-584 -> {"strings": [y_strings, z_strings], "shape": z.shape[-2:]}; order="wavefront" (codec.wave_order) adds "order" to it"""
        from ..codec import iframe_compress
        with torch.no_grad():
            return iframe_compress(self, x, order=order)

    def decompress(self, strings, shape, order="raster"):
        """priors.py:633-674 -> {"x_hat", "y_hat"}"""
        from ..codec import iframe_decompress
        with torch.no_grad():
            return iframe_decompress(self, strings, shape, order=order)

    def update(self, scale_table=None, force=False):
        """the Gaussian tables next to the bottleneck's (priors.py's MeanScaleHyperprior.update, which mbt2018 inherits)"""
        from .spatiotemporalpriors import get_scale_table
        if scale_table is None:
            scale_table = get_scale_table()
        updated = self.gaussian_conditional.update_scale_table(scale_table, force=force)
        updated |= super().update(force=force)
        return updated

    def load_state_dict(self, state_dict, strict=True):
        update_registered_buffers(self.gaussian_conditional, "gaussian_conditional",
                                  ["_quantized_cdf", "_offset", "_cdf_length", "scale_table"], state_dict)
        return super().load_state_dict(state_dict, strict=strict)


class MeanScaleHyperprior(CompressionModel):
    """Hyper-prior with a mean and a scale per latent and no spatial prior (priors.py:316-402, on ScaleHyperprior's g_a / g_s,
    :196-250): a whole frame's latents are coded in one host call (EntropyModel.compress / decompress on stem_symbols_pack /
    stem_symbols_unpack).  Module names and state-dict keys are the reference's."""

    def __init__(self, N, M, **kwargs):
        super().__init__(entropy_bottleneck_channels=N, **kwargs)
        self.g_a = FusedSequential(conv(3, N), GDN(N), conv(N, N), GDN(N), conv(N, N), GDN(N), conv(N, M))
        self.g_s = FusedSequential(deconv(M, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True),
                                   deconv(N, N), GDN(N, inverse=True), deconv(N, 3))
        self.h_a = FusedSequential(conv(M, N, stride=1, kernel_size=3), LeakyReLU(inplace=True),
                                   conv(N, N), LeakyReLU(inplace=True), conv(N, N))
        self.h_s = FusedSequential(deconv(N, M), LeakyReLU(inplace=True),
                                   deconv(M, M * 3 // 2), LeakyReLU(inplace=True),
                                   conv(M * 3 // 2, M * 2, stride=1, kernel_size=3))
        self.gaussian_conditional = GaussianConditional(None)
        self.N, self.M = int(N), int(M)

    @property
    def downsampling_factor(self) -> int:
        return 2 ** (4 + 2)

    def _gaussian_params(self, z_hat):
        return self.h_s(z_hat).chunk(2, 1)

    def forward(self, x):
        """priors.py:347-362 -> {"y", "y_hat", "x_hat", "likelihoods": {"y", "z"}}"""
        y = self.g_a(x)
        z = self.h_a(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        scales_hat, means_hat = self._gaussian_params(z_hat)
        y_hat, y_likelihoods = self.gaussian_conditional(y, scales_hat, means=means_hat)
        x_hat = self.g_s(y_hat)
        return {"y": y, "y_hat": y_hat, "x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods}}

    def compress(self, x):
        """priors.py:364-376 -> {"strings": [y_strings, z_strings], "shape": z.shape[-2:]}"""
        with torch.no_grad():
            y = self.g_a(x)
            z = self.h_a(y)
            z_strings = self.entropy_bottleneck.compress(z)
            z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
            scales_hat, means_hat = self._gaussian_params(z_hat)
            y_strings = self.gaussian_conditional.compress(y, None, means=means_hat, scales=scales_hat)
        return {"strings": [y_strings, z_strings], "shape": z.size()[-2:]}

    def decompress(self, strings, shape):
        """priors.py:378-388 -> {"x_hat", "y_hat"}"""
        assert isinstance(strings, list) and len(strings) == 2
        with torch.no_grad():
            z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
            scales_hat, means_hat = self._gaussian_params(z_hat)
            y_hat = self.gaussian_conditional.decompress(strings[0], None, means=means_hat, scales=scales_hat)
            x_hat = F.to_nchw(self.g_s(y_hat), clamp01=True)
        return {"x_hat": x_hat, "y_hat": y_hat}

    def getY(self, x):
        """-> (y, quantised y): noise in training mode, ROUNDED in eval mode (priors.py:390-395), unlike mbt2018's getY"""
        y = self.g_a(x)
        return y, self.gaussian_conditional.quantize(y, "noise" if self.training else "dequantize")

    def getX(self, y_hat):
        """g_s + clamp(0,1); returns a contiguous NCHW image batch (priors.py:397-402)"""
        return F.to_nchw(self.g_s(y_hat), clamp01=True)

    @classmethod
    def from_state_dict(cls, state_dict):
        """a new model sized by, and loaded from, `state_dict` (priors.py:278-285)"""
        net = cls(state_dict["g_a.0.weight"].size(0), state_dict["g_a.6.weight"].size(0))
        net.load_state_dict(state_dict)
        return net

    def update(self, scale_table=None, force=False):
        from .spatiotemporalpriors import get_scale_table
        if scale_table is None:
            scale_table = get_scale_table()
        updated = self.gaussian_conditional.update_scale_table(scale_table, force=force)
        updated |= super().update(force=force)
        return updated

    def load_state_dict(self, state_dict, strict=True):
        update_registered_buffers(self.gaussian_conditional, "gaussian_conditional",
                                  ["_quantized_cdf", "_offset", "_cdf_length", "scale_table"], state_dict)
        return super().load_state_dict(state_dict, strict=strict)


def _image_transforms(N, M):
    """g_a / g_s of the bmshj2018 and mbt2018-mean models (priors.py:124-142)"""
    g_a = FusedSequential(conv(3, N), GDN(N), conv(N, N), GDN(N), conv(N, N), GDN(N), conv(N, M))
    g_s = FusedSequential(deconv(M, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True),
                          deconv(N, N), GDN(N, inverse=True), deconv(N, 3))
    return g_a, g_s


class FactorizedPrior(CompressionModel):
    """Fully factorized prior (priors.py:109-181): the latents themselves go through an EntropyBottleneck of M channels, and a whole
    frame's latents are coded in one host call (EntropyBottleneck.compress / decompress).  Module names and state-dict keys are the
    reference's."""

    def __init__(self, N, M, **kwargs):
        super().__init__(entropy_bottleneck_channels=M, **kwargs)
        self.g_a, self.g_s = _image_transforms(N, M)
        self.N, self.M = int(N), int(M)

    @property
    def downsampling_factor(self) -> int:
        return 2 ** 4

    def forward(self, x):
        """priors.py:151-161 -> {"x_hat", "likelihoods": {"y"}} and, not in the reference, "y" / "y_hat" """
        y = self.g_a(x)
        y_hat, y_likelihoods = self.entropy_bottleneck(y)
        x_hat = self.g_s(y_hat)
        return {"y": y, "y_hat": y_hat, "x_hat": x_hat, "likelihoods": {"y": y_likelihoods}}

    def compress(self, x):
        """priors.py:172-175 -> {"strings": [y_strings], "shape": y.shape[-2:]}"""
        with torch.no_grad():
            y = self.g_a(x)
            y_strings = self.entropy_bottleneck.compress(y)
        return {"strings": [y_strings], "shape": y.size()[-2:]}

    def decompress(self, strings, shape):
        """priors.py:177-181 -> {"x_hat"} and, not in the reference, "y_hat" """
        assert isinstance(strings, list) and len(strings) == 1
        with torch.no_grad():
            y_hat = self.entropy_bottleneck.decompress(strings[0], shape)
            x_hat = F.to_nchw(self.g_s(y_hat), clamp01=True)
        return {"x_hat": x_hat, "y_hat": y_hat}

    @classmethod
    def from_state_dict(cls, state_dict):
        """a new model sized by, and loaded from, `state_dict` (priors.py:163-170)"""
        net = cls(state_dict["g_a.0.weight"].size(0), state_dict["g_a.6.weight"].size(0))
        net.load_state_dict(state_dict)
        return net


class ScaleHyperprior(CompressionModel):
    """Hyper-prior with a scale and NO mean per latent (priors.py:196-313): h_a reads |y|, ReLUs instead of leaky ReLUs (folded into
    the convolutions' epilogues), h_s ends in one, and the Gaussian likelihood is the zero-mean one (csrc/hyperprior.hip).  A whole
    frame's latents are coded in one host call, as in MeanScaleHyperprior.  Module names and state-dict keys are the reference's."""

    def __init__(self, N, M, **kwargs):
        super().__init__(entropy_bottleneck_channels=N, **kwargs)
        self.g_a, self.g_s = _image_transforms(N, M)
        self.h_a = FusedSequential(conv(M, N, stride=1, kernel_size=3), nn.ReLU(inplace=True),
                                   conv(N, N), nn.ReLU(inplace=True), conv(N, N))
        self.h_s = FusedSequential(deconv(N, N), nn.ReLU(inplace=True), deconv(N, N), nn.ReLU(inplace=True),
                                   conv(N, M, stride=1, kernel_size=3), nn.ReLU(inplace=True))
        self.gaussian_conditional = GaussianConditional(None)
        self.N, self.M = int(N), int(M)

    @property
    def downsampling_factor(self) -> int:
        return 2 ** (4 + 2)

    def _hyper_latents(self, y):
        return self.h_a(AbsFunction.apply(y))

    def forward(self, x):
        """priors.py:256-267 -> {"x_hat", "likelihoods": {"y", "z"}} and, not in the reference, "y" / "y_hat" / "entropy_params" """
        y = self.g_a(x)
        z = self._hyper_latents(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        scales_hat = self.h_s(z_hat)
        y_hat, y_likelihoods = self.gaussian_conditional(y, scales_hat)
        x_hat = self.g_s(y_hat)
        return {"y": y, "y_hat": y_hat, "x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods},
                "entropy_params": {"scales_hat": scales_hat}}

    def compress(self, x):
        """priors.py:294-304 -> {"strings": [y_strings, z_strings], "shape": z.shape[-2:]}"""
        with torch.no_grad():
            y = self.g_a(x)
            z = self._hyper_latents(y)
            z_strings = self.entropy_bottleneck.compress(z)
            z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
            scales_hat = self.h_s(z_hat)
            y_strings = self.gaussian_conditional.compress(y, None, scales=scales_hat)
        return {"strings": [y_strings, z_strings], "shape": z.size()[-2:]}

    def decompress(self, strings, shape):
        """priors.py:306-313 -> {"x_hat"} and, not in the reference, "y_hat" """
        assert isinstance(strings, list) and len(strings) == 2
        with torch.no_grad():
            z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
            scales_hat = self.h_s(z_hat)
            y_hat = self.gaussian_conditional.decompress(strings[0], None, scales=scales_hat)
            x_hat = F.to_nchw(self.g_s(y_hat), clamp01=True)
        return {"x_hat": x_hat, "y_hat": y_hat}

    @classmethod
    def from_state_dict(cls, state_dict):
        """a new model sized by, and loaded from, `state_dict` (priors.py:278-285)"""
        net = cls(state_dict["g_a.0.weight"].size(0), state_dict["g_a.6.weight"].size(0))
        net.load_state_dict(state_dict)
        return net

    def update(self, scale_table=None, force=False):
        from .spatiotemporalpriors import get_scale_table
        if scale_table is None:
            scale_table = get_scale_table()
        updated = self.gaussian_conditional.update_scale_table(scale_table, force=force)
        updated |= super().update(force=force)
        return updated

    def load_state_dict(self, state_dict, strict=True):
        update_registered_buffers(self.gaussian_conditional, "gaussian_conditional",
                                  ["_quantized_cdf", "_offset", "_cdf_length", "scale_table"], state_dict)
        return super().load_state_dict(state_dict, strict=strict)
