"""The cheng2020 I-frame models ("cheng2020-anchor", "cheng2020-attn": compressai/models/waseda.py:29-138): the entropy side of
JointAutoregressiveHierarchicalPriors (hyper-prior, masked context model, entropy-parameter network, M = N) around transforms
made of residual blocks with 3x3 / 1x1 convolutions and sub-pixel up-sampling (layers_residual.py).

Everything the STEM scripts and codec.py ask of an I-frame model is inherited: getY, getX, forward, compress, decompress, update,
load_state_dict, order="wavefront".  Module names and state-dict keys are the reference's.
"""
from ..layers import (AttentionBlock, BlockSequential, FusedSequential, LeakyReLU, ResidualBlock, ResidualBlockUpsample,
                      ResidualBlockWithStride, conv3x3, subpel_conv3x3)
from .priors import JointAutoregressiveHierarchicalPriors

__all__ = ["Cheng2020Anchor", "Cheng2020Attention"]


class Cheng2020Anchor(JointAutoregressiveHierarchicalPriors):
    """waseda.py:29-96"""

    def __init__(self, N=192, **kwargs):
        super().__init__(N=N, M=N, **kwargs)
        self.g_a = BlockSequential(ResidualBlockWithStride(3, N, stride=2), ResidualBlock(N, N),
                                   ResidualBlockWithStride(N, N, stride=2), ResidualBlock(N, N),
                                   ResidualBlockWithStride(N, N, stride=2), ResidualBlock(N, N),
                                   conv3x3(N, N, stride=2))
        self.h_a = FusedSequential(conv3x3(N, N), LeakyReLU(inplace=True), conv3x3(N, N), LeakyReLU(inplace=True),
                                   conv3x3(N, N, stride=2), LeakyReLU(inplace=True), conv3x3(N, N), LeakyReLU(inplace=True),
                                   conv3x3(N, N, stride=2))
        self.h_s = BlockSequential(conv3x3(N, N), LeakyReLU(inplace=True), subpel_conv3x3(N, N, 2), LeakyReLU(inplace=True),
                                   conv3x3(N, N * 3 // 2), LeakyReLU(inplace=True), subpel_conv3x3(N * 3 // 2, N * 3 // 2, 2),
                                   LeakyReLU(inplace=True), conv3x3(N * 3 // 2, N * 2))
        self.g_s = BlockSequential(ResidualBlock(N, N), ResidualBlockUpsample(N, N, 2), ResidualBlock(N, N),
                                   ResidualBlockUpsample(N, N, 2), ResidualBlock(N, N), ResidualBlockUpsample(N, N, 2),
                                   ResidualBlock(N, N), subpel_conv3x3(N, 3, 2))
        # key ORDER of the reference's state dict: there gaussian_conditional is registered (by MeanScaleHyperprior.__init__,
        # compressai/models/priors.py) before the entropy-parameter network and the context model
        for k in ("entropy_parameters", "context_prediction"):
            self._modules[k] = self._modules.pop(k)

    @classmethod
    def from_state_dict(cls, state_dict):
        """a new model sized by, and loaded from, `state_dict` (waseda.py:90-96)"""
        net = cls(state_dict["g_a.0.conv1.weight"].size(0))
        net.load_state_dict(state_dict)
        return net


class Cheng2020Attention(Cheng2020Anchor):
    """waseda.py:99-138: the anchor model with attention blocks at 1/4 and 1/16 resolution of both transforms"""

    def __init__(self, N=192, **kwargs):
        super().__init__(N=N, **kwargs)
        self.g_a = BlockSequential(ResidualBlockWithStride(3, N, stride=2), ResidualBlock(N, N),
                                   ResidualBlockWithStride(N, N, stride=2), AttentionBlock(N), ResidualBlock(N, N),
                                   ResidualBlockWithStride(N, N, stride=2), ResidualBlock(N, N),
                                   conv3x3(N, N, stride=2), AttentionBlock(N))
        self.g_s = BlockSequential(AttentionBlock(N), ResidualBlock(N, N), ResidualBlockUpsample(N, N, 2), ResidualBlock(N, N),
                                   ResidualBlockUpsample(N, N, 2), AttentionBlock(N), ResidualBlock(N, N),
                                   ResidualBlockUpsample(N, N, 2), ResidualBlock(N, N), subpel_conv3x3(N, 3, 2))
