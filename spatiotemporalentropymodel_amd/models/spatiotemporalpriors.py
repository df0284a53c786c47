"""The five STEM P-frame entropy models with the reference's constructor signature, module names,
state-dict keys and method contracts (compressai/models/spatiotemporalpriors.py:33-1072):

    forward(y_cur, y_conditioned)    -> {"y_hat", "likelihoods": {"y", "z"}}
    compress(y_cur, y_conditioned)   -> {"strings": [y_strings, z_strings], "shape": z.shape[-2:]}
    decompress(strings, shape, y_conditioned) -> Tensor  (dict {"y_hat"} for the _Res model, as upstream)
    update(scale_table=None, force=False), load_state_dict, aux_loss

forward / backward run the fused HIP schedule of `engine.StemEngine`; the bitstream side keeps the
rANS coder on the host (codec.py).
"""
import torch
import torch.nn as nn

from .. import functional as F
from ..engine import StemEngine, StemFunction
from ..entropy_models import GaussianConditional
from ..layers import CatFunction, Conv2d, ConvTranspose2d, FusedSequential, LeakyReLU, MaskedConv2d
from .priors import CompressionModel, get_scale_table      # get_scale_table: re-exported, it lives next to ScaleHyperprior

__all__ = ["get_scale_table", "SpatioTemporalPriorModelWithoutSPMTPM", "SpatioTemporalPriorModelWithoutSPM",
           "SpatioTemporalPriorModelWithoutTPM", "SpatioTemporalPriorModel", "SpatioTemporalPriorModel_Res"]

def _tpm(cin):
    return FusedSequential(Conv2d(cin, 256, kernel_size=5, padding=2, stride=1), LeakyReLU(),
                           Conv2d(256, 320, kernel_size=5, padding=2, stride=1), LeakyReLU(),
                           Conv2d(320, cin * 2, kernel_size=5, padding=2, stride=1))


def _he(cin, zc):
    return FusedSequential(Conv2d(cin * 2, 256, kernel_size=3, padding=1, stride=1), LeakyReLU(),
                           Conv2d(256, 256, kernel_size=5, padding=2, stride=2), LeakyReLU(),
                           Conv2d(256, zc, kernel_size=5, padding=2, stride=2))


def _hd(cin, zc):
    return FusedSequential(ConvTranspose2d(zc, 256, kernel_size=5, padding=2, stride=2, output_padding=1), LeakyReLU(),
                           ConvTranspose2d(256, 256, kernel_size=5, padding=2, stride=2, output_padding=1), LeakyReLU(),
                           Conv2d(256, cin * 2, kernel_size=3, padding=1, stride=1))


def _epm(cin, nprior):
    return FusedSequential(Conv2d(cin * 2 * nprior, 768, kernel_size=1), LeakyReLU(),
                           Conv2d(768, 576, kernel_size=1), LeakyReLU(),
                           Conv2d(576, cin * 2, kernel_size=1))


class _StemBase(CompressionModel):
    HAS_TPM = HAS_SPM = RESIDUAL = False
    HARD_CODED_Z = False          # the two ablations without SPM hard-code 256 hyper-latent channels (:44-58,150-164)
    DECOMPRESS_RETURNS_DICT = False

    def __init__(self, entropy_bottleneck_channels=256, in_channels=192):
        super().__init__(entropy_bottleneck_channels=entropy_bottleneck_channels)
        zc = 256 if self.HARD_CODED_Z else entropy_bottleneck_channels
        # module creation order follows the reference so that parameter / state-dict order is identical
        if self.HAS_TPM:
            self.TPM = _tpm(in_channels)
        self.HE = _he(in_channels, zc)
        self.HD = _hd(in_channels, zc)
        if self.HAS_SPM:
            self.context_prediction = MaskedConv2d(in_channels, in_channels * 2, kernel_size=5, padding=2, stride=1)
        self.EPM = _epm(in_channels, 1 + int(self.HAS_TPM) + int(self.HAS_SPM))
        self.gaussian_conditional = GaussianConditional(None)
        self.in_channels = in_channels
        self._engine = None
        self._engine_params = None

    # ---- fused forward -----------------------------------------------------------------------
    def engine(self) -> StemEngine:
        if self._engine is None:
            object.__setattr__(self, "_engine", StemEngine(self, self.HAS_TPM, self.HAS_SPM, self.RESIDUAL))
            object.__setattr__(self, "_engine_params", [p for n, p in self.named_parameters() if not n.endswith(".quantiles")])
        return self._engine

    def _forward_modules(self, y_cur, y_conditioned):
        """The reference's forward module by module (spatiotemporalpriors.py:70-83, 176-194, 291-309, 561-585, 845-868), every module
        on its own kernels and autograd node: the route of a model whose bottleneck the fused schedule does not know."""
        gc = self.gaussian_conditional
        z = self.HE(CatFunction.apply(y_cur, y_conditioned))
        z_hat, lik_z = self.entropy_bottleneck(z)
        priors = ([self.TPM(y_conditioned)] if self.HAS_TPM else []) + [self.HD(z_hat)]
        target = F.sub(F.dense_nhwc(y_cur.detach()), F.dense_nhwc(y_conditioned.detach())) if self.RESIDUAL else y_cur
        if self.HAS_SPM:
            t_hat = gc.quantize(target.detach(), "noise" if self.training else "dequantize")
            priors.append(self.context_prediction(t_hat))
        gp = self.EPM(CatFunction.apply(*priors) if len(priors) > 1 else priors[0])
        scales_hat, means_hat = gp.chunk(2, 1)
        out, lik_y = gc(target, scales_hat, means=means_hat)
        if self.HAS_SPM:
            y_hat = F.add(t_hat, F.dense_nhwc(y_conditioned.detach())) if self.RESIDUAL else t_hat
        else:
            y_hat = out
        return {"y_hat": y_hat, "likelihoods": {"y": lik_y, "z": lik_z}}

    def forward(self, y_cur, y_conditioned):
        if tuple(self.entropy_bottleneck.filters) != (3, 3, 3, 3):
            return self._forward_modules(y_cur, y_conditioned)
        eng = self.engine()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._engine_params):
            y_hat, lik_y, lik_z = StemFunction.apply(eng, self.training, y_cur, y_conditioned, *self._engine_params)
        else:
            y_hat, lik_y, lik_z, _ = eng.forward(y_cur, y_conditioned, self.training)
        return {"y_hat": y_hat, "likelihoods": {"y": lik_y, "z": lik_z}}

    # ---- bitstream side ----------------------------------------------------------------------
    def compress(self, y_cur, y_conditioned, order="raster", return_y_hat=False):
        """order: "raster" (the reference's) or "wavefront" (codec.wave_order; the result then carries "order").  return_y_hat=True: the
        result also carries "y_hat", the latent `decompress` of these strings returns, from the encoder's own state (no decoder runs)"""
        from ..codec import stem_compress
        return stem_compress(self, y_cur, y_conditioned, order=order, return_y_hat=return_y_hat)

    def decompress(self, strings, shape, y_conditioned, order="raster"):
        from ..codec import stem_decompress
        assert isinstance(strings, list) and len(strings) == 2
        y_hat = stem_decompress(self, strings, shape, y_conditioned, order=order)
        return {"y_hat": y_hat} if self.DECOMPRESS_RETURNS_DICT else y_hat


class SpatioTemporalPriorModelWithoutSPMTPM(_StemBase):
    """Hyper-prior only (spatiotemporalpriors.py:33-129)."""
    HARD_CODED_Z = True


class SpatioTemporalPriorModelWithoutSPM(_StemBase):
    """Hyper-prior + temporal prior (spatiotemporalpriors.py:132-243)."""
    HAS_TPM = True
    HARD_CODED_Z = True


class SpatioTemporalPriorModelWithoutTPM(_StemBase):
    """Hyper-prior + spatial (masked-conv) prior (spatiotemporalpriors.py:246-505)."""
    HAS_SPM = True


class SpatioTemporalPriorModel(_StemBase):
    """Hyper + temporal + spatial priors on y_cur (spatiotemporalpriors.py:508-788)."""
    HAS_TPM = HAS_SPM = True


class SpatioTemporalPriorModel_Res(_StemBase):
    """Hyper + temporal + spatial priors on the residual y_cur - y_conditioned (spatiotemporalpriors.py:791-1072)."""
    HAS_TPM = HAS_SPM = RESIDUAL = True
    DECOMPRESS_RETURNS_DICT = True
