"""Name -> constructor registry (compressai/zoo/__init__.py:17-24, compressai/zoo/image.py:131-215) for the
architectures the STEM scripts instantiate: `models["mbt2018"](quality=4)` (stem/trainSTEM.py:113),
`models["mbt2018-mean"](quality=4)` (stem_roi/eval_stem_baseline.py:294-297), the two stronger intra codecs their `--model`
argument reaches, `models["cheng2020-anchor"]` / `models["cheng2020-attn"]` (stem_roi/train_stem_roi.py:123), and the two
zero-mean models that complete the reference's registry and the container's model ids (bitstream.MODEL_NAMES 0 and 1),
`models["bmshj2018-factorized"]` / `models["bmshj2018-hyperprior"]`.  `models` lists the six names in the reference's order."""
from .models.priors import FactorizedPrior, JointAutoregressiveHierarchicalPriors, MeanScaleHyperprior, ScaleHyperprior
from .models.waseda import Cheng2020Anchor, Cheng2020Attention

cfgs = {"bmshj2018-factorized": {1: (128, 192), 2: (128, 192), 3: (128, 192), 4: (128, 192), 5: (128, 192),
                                 6: (192, 320), 7: (192, 320), 8: (192, 320)},
        "bmshj2018-hyperprior": {1: (128, 192), 2: (128, 192), 3: (128, 192), 4: (128, 192), 5: (128, 192),
                                 6: (192, 320), 7: (192, 320), 8: (192, 320)},
        "mbt2018": {1: (192, 192), 2: (192, 192), 3: (192, 192), 4: (192, 192),
                    5: (192, 320), 6: (192, 320), 7: (192, 320), 8: (192, 320)},
        "mbt2018-mean": {1: (128, 192), 2: (128, 192), 3: (128, 192), 4: (128, 192),
                         5: (192, 320), 6: (192, 320), 7: (192, 320), 8: (192, 320)},
        "cheng2020-anchor": {1: (128,), 2: (128,), 3: (128,), 4: (192,), 5: (192,), 6: (192,)},
        "cheng2020-attn": {1: (128,), 2: (128,), 3: (128,), 4: (192,), 5: (192,), 6: (192,)}}


def _build(arch, cls, quality, metric, pretrained, kwargs):
    if metric not in ("mse",):
        raise ValueError(f'Invalid metric "{metric}"')
    if quality not in cfgs[arch]:
        raise ValueError(f'Invalid quality "{quality}", should be between (1, {max(cfgs[arch])})')
    if pretrained:
        raise RuntimeError("pretrained weights are downloaded from S3 by the reference (zoo/image.py:46); no network here")
    return cls(*cfgs[arch][quality], **kwargs)


def bmshj2018_factorized(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    return _build("bmshj2018-factorized", FactorizedPrior, quality, metric, pretrained, kwargs)


def bmshj2018_hyperprior(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    return _build("bmshj2018-hyperprior", ScaleHyperprior, quality, metric, pretrained, kwargs)


def mbt2018(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    return _build("mbt2018", JointAutoregressiveHierarchicalPriors, quality, metric, pretrained, kwargs)


def mbt2018_mean(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    return _build("mbt2018-mean", MeanScaleHyperprior, quality, metric, pretrained, kwargs)


def cheng2020_anchor(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    return _build("cheng2020-anchor", Cheng2020Anchor, quality, metric, pretrained, kwargs)


def cheng2020_attn(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    return _build("cheng2020-attn", Cheng2020Attention, quality, metric, pretrained, kwargs)


models = {"bmshj2018-factorized": bmshj2018_factorized, "bmshj2018-hyperprior": bmshj2018_hyperprior, "mbt2018-mean": mbt2018_mean,
          "mbt2018": mbt2018, "cheng2020-anchor": cheng2020_anchor, "cheng2020-attn": cheng2020_attn}
