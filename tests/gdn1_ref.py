"""GDN1 (the simplified normalisation, compressai/layers/gdn.py:70-96) in float64 numpy: the project's own statement of the formulas
of include/stem_gdn1.h, which the kernel tests compare with.  tests/test_gdn1_ref.py pins it against the reference's own module
(tests/golden/gdn1.npz).

Pixels are rows: x, dy, y, dx are [npix, C]; beta [C] and gamma [C, C] are the STORED parameters, row i of gamma = output channel i."""
import numpy as np

PEDESTAL = 2.0 ** -36
GAMMA_BOUND = 2.0 ** -18


def beta_bound(beta_min):
    return (float(beta_min) + PEDESTAL) ** 0.5


def reparam(v, bound):
    """NonNegativeParametrizer.forward (ops/parametrizers.py:42-45): max(v, bound)^2 - 2^-36"""
    return np.maximum(np.asarray(v, np.float64), bound) ** 2 - PEDESTAL


def reparam_backward(v, dprime, bound):
    """gradient wrt the stored value: 2 max(v, bound) d', passed iff v >= bound or it is negative (ops/bound_ops.py:28-31)"""
    v = np.asarray(v, np.float64)
    g = 2.0 * np.maximum(v, bound) * dprime
    return np.where((v >= bound) | (g < 0), g, 0.0)


def norm(x, beta, gamma, beta_min=1e-6):
    """n[p][i] = beta'[i] + sum_j gamma'[i][j] |x[p][j]|"""
    x = np.asarray(x, np.float64)
    return reparam(beta, beta_bound(beta_min))[None, :] + np.abs(x) @ reparam(gamma, GAMMA_BOUND).T


def forward(x, beta, gamma, inverse=False, beta_min=1e-6):
    x = np.asarray(x, np.float64)
    n = norm(x, beta, gamma, beta_min)
    return x * n if inverse else x * (1.0 / n)


def backward(x, dy, beta, gamma, inverse=False, beta_min=1e-6):
    """-> dx, dbeta, dgamma (stored parameters), dbeta', dgamma' (reparametrised ones)"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n = norm(x, beta, gamma, beta_min)
    if inverse:
        u, g = dy * n, dy * x
    else:
        r = 1.0 / n
        u, g = dy * r, -dy * x * r * r
    gp = reparam(gamma, GAMMA_BOUND)
    dx = u + np.sign(x) * (g @ gp)                  # np.sign(+-0) = 0, as torch.abs's derivative
    dgp, dbp = g.T @ np.abs(x), g.sum(axis=0)
    return dx, reparam_backward(beta, dbp, beta_bound(beta_min)), reparam_backward(gamma, dgp, GAMMA_BOUND), dbp, dgp
