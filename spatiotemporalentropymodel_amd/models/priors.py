"""CompressionModel base class and the reference's chain of image models (compressai/models/priors.py): FactorizedPrior
("bmshj2018-factorized", :109-181), ScaleHyperprior ("bmshj2018-hyperprior", :196-313) -> MeanScaleHyperprior ("mbt2018-mean",
:316-402) -> JointAutoregressiveHierarchicalPriors ("mbt2018", :406-694), the I-frame model of the STEM scripts (-> the cheng2020
models, models/waseda.py).  ScaleHyperprior holds what the chain shares; a subclass states its modules through the builders its
constructor calls, so every layer is made once and in the reference's order.

On the STEM training path only g_a / g_s (getY / getX) are executed.  The evaluation loop also codes its I frames with these models
(stem/evalSTEM.py:54-59: compress / decompress): the hyper-prior models code a whole frame's latents in one host call, mbt2018 with the
same raster-order coder as the STEM models (codec.py: the entropy-parameter network sees cat(params, ctx) exactly like a STEM model
without temporal prior).
"""
import math

import torch
import torch.nn as nn

from .. import functional as F
from ..entropy_models import EntropyBottleneck, GaussianConditional
from ..layers import GDN, AbsFunction, Conv2d, ConvTranspose2d, FusedSequential, LeakyReLU, MaskedConv2d, cat, conv, deconv
from .utils import update_registered_buffers

__all__ = ["CompressionModel", "JointAutoregressiveHierarchicalPriors", "MeanScaleHyperprior", "FactorizedPrior", "ScaleHyperprior"]

# From Balle's tensorflow compression examples (priors.py:31-39)
SCALES_MIN = 0.11
SCALES_MAX = 256
SCALES_LEVELS = 64


def get_scale_table(min=SCALES_MIN, max=SCALES_MAX, levels=SCALES_LEVELS):  # pylint: disable=W0622
    return torch.exp(torch.linspace(math.log(min), math.log(max), levels))


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

    def update(self, scale_table=None, force=False):
        """the bottlenecks' tables and, for a model with a `gaussian_conditional`, the Gaussian tables next to them (priors.py:74-96,
        287-292); scale_table: `get_scale_table()` by default"""
        updated = False
        if hasattr(self, "gaussian_conditional"):
            updated = self.gaussian_conditional.update_scale_table(get_scale_table() if scale_table is None else scale_table, force=force)
        for m in self.children():
            if not isinstance(m, EntropyBottleneck):
                continue
            updated |= m.update(force=force)
        return updated

    def load_state_dict(self, state_dict, strict=True):
        if hasattr(self, "gaussian_conditional"):
            update_registered_buffers(self.gaussian_conditional, "gaussian_conditional",
                                      ["_quantized_cdf", "_offset", "_cdf_length", "scale_table"], state_dict)
        update_registered_buffers(self.entropy_bottleneck, "entropy_bottleneck",
                                  ["_quantized_cdf", "_offset", "_cdf_length"], state_dict)
        return super().load_state_dict(state_dict, strict=strict)


def _image_transforms(N, M):
    """g_a / g_s of the bmshj2018 and mbt2018 models (priors.py:124-142)"""
    g_a = FusedSequential(conv(3, N), GDN(N), conv(N, N), GDN(N), conv(N, N), GDN(N), conv(N, M))
    g_s = FusedSequential(deconv(M, N), GDN(N, inverse=True), deconv(N, N), GDN(N, inverse=True),
                          deconv(N, N), GDN(N, inverse=True), deconv(N, 3))
    return g_a, g_s


def _from_state_dict(cls, state_dict):
    """a new model sized by, and loaded from, `state_dict` (priors.py:163-170, 278-285): N and M are g_a's first and last widths"""
    net = cls(state_dict["g_a.0.weight"].size(0), state_dict["g_a.6.weight"].size(0))
    net.load_state_dict(state_dict)
    return net


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

    def compress(self, x, return_y_hat=False):
        """priors.py:172-175 -> {"strings": [y_strings], "shape": y.shape[-2:]}; return_y_hat=True adds "y_hat", what `decompress` of the
        strings returns as "y_hat", from the symbols the encoder still holds on the device"""
        with torch.no_grad():
            y = self.g_a(x)
            if return_y_hat:
                y_strings, y_hat = self.entropy_bottleneck.compress(y, return_y_hat=True)
                return {"strings": [y_strings], "shape": y.size()[-2:], "y_hat": y_hat}
            y_strings = self.entropy_bottleneck.compress(y)
        return {"strings": [y_strings], "shape": y.size()[-2:]}

    def decompress(self, strings, shape, latents_only=False):
        """priors.py:177-181 -> {"x_hat"} and, not in the reference, "y_hat"; latents_only=True: {"y_hat"} alone, g_s does not run"""
        assert isinstance(strings, list) and len(strings) == 1
        with torch.no_grad():
            y_hat = self.entropy_bottleneck.decompress(strings[0], shape)
            if latents_only:
                return {"y_hat": y_hat}
            x_hat = F.to_nchw(self.g_s(y_hat), clamp01=True)
        return {"x_hat": x_hat, "y_hat": y_hat}

    from_state_dict = classmethod(_from_state_dict)


class ScaleHyperprior(CompressionModel):
    """Hyper-prior with a scale and NO mean per latent (priors.py:196-313): h_a reads |y|, ReLUs instead of leaky ReLUs (folded into
    the convolutions' epilogues), h_s ends in one, and the Gaussian likelihood is the zero-mean one (csrc/hyperprior.hip).  A whole
    frame's latents are coded in one host call (EntropyModel.compress / decompress on stem_symbols_pack / stem_symbols_unpack).
    Module names and state-dict keys are the reference's, here and in the subclasses.  What a subclass changes: `_hyper_transforms`,
    `_context_modules` (what it builds and in which place) and, for the one-shot coder, `_hyper_input` and `_gaussian_params`."""

    def __init__(self, N, M, **kwargs):
        super().__init__(entropy_bottleneck_channels=N, **kwargs)
        self.g_a, self.g_s = _image_transforms(N, M)
        self.h_a, self.h_s = self._hyper_transforms(N, M)
        self._context_modules(M)
        self.gaussian_conditional = GaussianConditional(None)
        self.N, self.M = int(N), int(M)

    def _hyper_transforms(self, N, M):
        """-> (h_a, h_s), built in this order"""
        return (FusedSequential(conv(M, N, stride=1, kernel_size=3), nn.ReLU(inplace=True), conv(N, N), nn.ReLU(inplace=True), conv(N, N)),
                FusedSequential(deconv(N, N), nn.ReLU(inplace=True), deconv(N, N), nn.ReLU(inplace=True),
                                conv(N, M, stride=1, kernel_size=3), nn.ReLU(inplace=True)))

    def _context_modules(self, M):
        """modules registered between h_s and gaussian_conditional: none but mbt2018's"""

    @property
    def downsampling_factor(self) -> int:
        return 2 ** (4 + 2)

    def _hyper_input(self, y):
        """what h_a reads"""
        return AbsFunction.apply(y)

    def _gaussian_params(self, z_hat):
        """-> (scales_hat, means_hat or None)"""
        return self.h_s(z_hat), None

    def forward(self, x):
        """priors.py:256-267 -> {"x_hat", "likelihoods": {"y", "z"}} and, not in the reference, "y" / "y_hat" / "entropy_params" """
        y = self.g_a(x)
        z = self.h_a(self._hyper_input(y))
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        scales_hat = self.h_s(z_hat)
        y_hat, y_likelihoods = self.gaussian_conditional(y, scales_hat)
        x_hat = self.g_s(y_hat)
        return {"y": y, "y_hat": y_hat, "x_hat": x_hat, "likelihoods": {"y": y_likelihoods, "z": z_likelihoods},
                "entropy_params": {"scales_hat": scales_hat}}

    def compress(self, x, return_y_hat=False):
        """priors.py:294-304, 364-376 -> {"strings": [y_strings, z_strings], "shape": z.shape[-2:]}; return_y_hat=True adds "y_hat", what
        `decompress` of the strings returns as "y_hat", from the symbols the encoder still holds on the device"""
        with torch.no_grad():
            y = self.g_a(x)
            z = self.h_a(self._hyper_input(y))
            z_strings = self.entropy_bottleneck.compress(z)
            z_hat = self.entropy_bottleneck.decompress(z_strings, z.size()[-2:])
            scales_hat, means_hat = self._gaussian_params(z_hat)
            if return_y_hat:
                y_strings, y_hat = self.gaussian_conditional.compress(y, None, means=means_hat, scales=scales_hat, return_y_hat=True)
                return {"strings": [y_strings, z_strings], "shape": z.size()[-2:], "y_hat": y_hat}
            y_strings = self.gaussian_conditional.compress(y, None, means=means_hat, scales=scales_hat)
        return {"strings": [y_strings, z_strings], "shape": z.size()[-2:]}

    def decompress(self, strings, shape, latents_only=False):
        """priors.py:306-313, 378-388 -> {"x_hat"} and, not in the reference's ScaleHyperprior, "y_hat"; latents_only=True: {"y_hat"}
        alone, g_s does not run"""
        assert isinstance(strings, list) and len(strings) == 2
        with torch.no_grad():
            z_hat = self.entropy_bottleneck.decompress(strings[1], shape)
            scales_hat, means_hat = self._gaussian_params(z_hat)
            y_hat = self.gaussian_conditional.decompress(strings[0], None, means=means_hat, scales=scales_hat)
            if latents_only:
                return {"y_hat": y_hat}
            x_hat = F.to_nchw(self.g_s(y_hat), clamp01=True)
        return {"x_hat": x_hat, "y_hat": y_hat}

    from_state_dict = classmethod(_from_state_dict)


class MeanScaleHyperprior(ScaleHyperprior):
    """Hyper-prior with a mean and a scale per latent and no spatial prior (priors.py:316-402): h_a reads y itself, leaky ReLUs, and
    h_s gives 2 M channels, the scales and the means."""

    def _hyper_transforms(self, N, M):
        return (FusedSequential(conv(M, N, stride=1, kernel_size=3), LeakyReLU(inplace=True), conv(N, N), LeakyReLU(inplace=True), conv(N, N)),
                FusedSequential(deconv(N, M), LeakyReLU(inplace=True), deconv(M, M * 3 // 2), LeakyReLU(inplace=True),
                                conv(M * 3 // 2, M * 2, stride=1, kernel_size=3)))

    def _hyper_input(self, y):
        return y

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

    # ---- the two entry points the STEM scripts use (priors.py:390-402, 686-694) ---------------
    def getY(self, x):
        """-> (y, quantised y): noise in training mode, ROUNDED in eval mode (priors.py:390-395), unlike mbt2018's getY"""
        y = self.g_a(x)
        return y, self.gaussian_conditional.quantize(y, "noise" if self.training else "dequantize")

    def getX(self, y_hat):
        """g_s + clamp(0,1); returns a contiguous NCHW image batch (layout change and clamp fused; priors.py:397-402)"""
        return F.to_nchw(self.g_s(y_hat), clamp01=True)


class JointAutoregressiveHierarchicalPriors(MeanScaleHyperprior):
    """mbt2018-mean's transforms plus a masked context model and an entropy-parameter network that joins it with the hyper-prior
    (priors.py:406-694); the latents are coded position by position (codec.py).  The two modules are registered in front of
    gaussian_conditional, where this project's mbt2018 checkpoints and the optimisers' flat buffers have them."""

    def __init__(self, N=192, M=192, **kwargs):
        super().__init__(N, M, **kwargs)

    def _context_modules(self, M):
        self.entropy_parameters = FusedSequential(Conv2d(M * 12 // 3, M * 10 // 3, 1), LeakyReLU(inplace=True),
                                                  Conv2d(M * 10 // 3, M * 8 // 3, 1), LeakyReLU(inplace=True),
                                                  Conv2d(M * 8 // 3, M * 6 // 3, 1))
        self.context_prediction = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)

    def getY(self, x):
        """-> (y, y + U(-1/2,1/2)); the mbt2018 variant adds noise in eval mode too (priors.py:691)."""
        y = self.g_a(x)
        y_quantized = self.gaussian_conditional.quantize(y, "noise")
        return y, y_quantized

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

    def compress(self, x, order="raster", return_y_hat=False):
        """priors.py:544-584 -> {"strings": [y_strings, z_strings], "shape": z.shape[-2:]}; order="wavefront" (codec.wave_order) adds "order" to
        it, return_y_hat=True "y_hat": the latent `decompress` returns, left by the coding kernels in their buffer (no decoder runs)"""
        from ..codec import iframe_compress
        with torch.no_grad():
            return iframe_compress(self, x, order=order, return_y_hat=return_y_hat)

    def decompress(self, strings, shape, order="raster"):
        """priors.py:633-674 -> {"x_hat", "y_hat"}"""
        from ..codec import iframe_decompress
        with torch.no_grad():
            return iframe_decompress(self, strings, shape, order=order)
