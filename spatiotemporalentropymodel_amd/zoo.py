"""Name -> constructor registry (compressai/zoo/__init__.py:17-24, compressai/zoo/image.py:131-215) for the
two architectures the STEM scripts instantiate: `models["mbt2018"](quality=4)` (stem/trainSTEM.py:113) and
`models["mbt2018-mean"](quality=4)` (stem_roi/eval_stem_baseline.py:294-297)."""
from .models.priors import JointAutoregressiveHierarchicalPriors, MeanScaleHyperprior

cfgs = {"mbt2018": {1: (192, 192), 2: (192, 192), 3: (192, 192), 4: (192, 192),
                    5: (192, 320), 6: (192, 320), 7: (192, 320), 8: (192, 320)},
        "mbt2018-mean": {1: (128, 192), 2: (128, 192), 3: (128, 192), 4: (128, 192),
                         5: (192, 320), 6: (192, 320), 7: (192, 320), 8: (192, 320)}}


def _build(arch, cls, quality, metric, pretrained, kwargs):
    if metric not in ("mse",):
        raise ValueError(f'Invalid metric "{metric}"')
    if quality not in cfgs[arch]:
        raise ValueError(f'Invalid quality "{quality}", should be between (1, 8)')
    if pretrained:
        raise RuntimeError("pretrained weights are downloaded from S3 by the reference (zoo/image.py:46); no network here")
    return cls(*cfgs[arch][quality], **kwargs)


def mbt2018(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    return _build("mbt2018", JointAutoregressiveHierarchicalPriors, quality, metric, pretrained, kwargs)


def mbt2018_mean(quality, metric="mse", pretrained=False, progress=True, **kwargs):
    return _build("mbt2018-mean", MeanScaleHyperprior, quality, metric, pretrained, kwargs)


models = {"mbt2018": mbt2018, "mbt2018-mean": mbt2018_mean}
