"""Float64 statements of the fp32-MFMA family's operations (csrc/igemm.hip, csrc/wgrad.hip), in plain numpy: nothing here
comes from the library.  Tensors are NCHW, weights [K,C,R,S] (Conv2d) or [C,K,R,S] (ConvTranspose2d), every result float64.
Pinned on the CPU by tests/test_conv_ref.py (CPU oracle, golden vectors of the reference); tests/test_hip_fp32_plans.py
compares the kernels with these.

Every convolution-shaped operation is stated through three tap loops over a zero-padded input:
    forward   y[b,k,oy,ox]  = sum_{r,s,c} xp[b,c,oy*st+r,ox*st+s] * w[k,c,r,s]
    adjoint   dxp[b,c,oy*st+r,ox*st+s] += dy[b,k,oy,ox] * w[k,c,r,s]
    weights   dw[k,c,r,s]   = sum_{b,oy,ox} dy[b,k,oy,ox] * xp[b,c,oy*st+r,ox*st+s]
A transposed convolution is the adjoint of the convolution that maps its output grid to its input grid.
"""
import numpy as np

PEDESTAL = 2.0 ** -36                  # reparametrisation pedestal (parametrizers.py); gamma's bound is its square root, 2^-18
GAMMA_BOUND = 2.0 ** -18


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def conv_out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def deconv_out_hw(H, W, R, S, stride, pad, opad):
    return (H - 1) * stride - 2 * pad + R + opad, (W - 1) * stride - 2 * pad + S + opad


def _padded(x, pad):
    return np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))


def _window(xp, r, s, OH, OW, stride):
    return xp[:, :, r:r + stride * (OH - 1) + 1:stride, s:s + stride * (OW - 1) + 1:stride]


def conv2d_fwd(x, w, b, stride, pad):
    x, w, b = _f64(x), _f64(w), _f64(b)
    K, C, R, S = w.shape
    OH, OW = conv_out_hw(x.shape[2], x.shape[3], R, S, stride, pad)
    xp = _padded(x, pad)
    y = np.zeros((x.shape[0], K, OH, OW))
    for r in range(R):
        for s in range(S):
            y += np.einsum("bchw,kc->bkhw", _window(xp, r, s, OH, OW, stride), w[:, :, r, s])
    return y if b is None else y + b[None, :, None, None]


def conv2d_dx(dy, w, x_shape, stride, pad):
    """input gradient of conv2d_fwd for an input of shape x_shape"""
    dy, w = _f64(dy), _f64(w)
    K, C, R, S = w.shape
    B, Cx, H, W = x_shape
    OH, OW = conv_out_hw(H, W, R, S, stride, pad)
    assert Cx == C and dy.shape == (B, K, OH, OW), (dy.shape, (B, K, OH, OW))
    dxp = np.zeros((B, C, H + 2 * pad, W + 2 * pad))
    for r in range(R):
        for s in range(S):
            _window(dxp, r, s, OH, OW, stride)[...] += np.einsum("bkhw,kc->bchw", dy, w[:, :, r, s])
    return dxp[:, :, pad:pad + H, pad:pad + W]


def conv2d_dw(x, dy, R, S, stride, pad):
    """weight gradient [K,C,R,S] of conv2d_fwd"""
    x, dy = _f64(x), _f64(dy)
    OH, OW = dy.shape[2], dy.shape[3]
    assert (OH, OW) == conv_out_hw(x.shape[2], x.shape[3], R, S, stride, pad)
    xp = _padded(x, pad)
    dw = np.zeros((dy.shape[1], x.shape[1], R, S))
    for r in range(R):
        for s in range(S):
            dw[:, :, r, s] = np.einsum("bkhw,bchw->kc", dy, _window(xp, r, s, OH, OW, stride))
    return dw


def bias_grad(dy):
    return _f64(dy).sum(axis=(0, 2, 3))


def deconv2d_fwd(x, w, b, stride, pad, opad):
    """ConvTranspose2d: x [B,C,H,W], w [C,K,R,S] -> [B,K,Hd,Wd]"""
    x, w, b = _f64(x), _f64(w), _f64(b)
    C, K, R, S = w.shape
    Hd, Wd = deconv_out_hw(x.shape[2], x.shape[3], R, S, stride, pad, opad)
    y = conv2d_dx(x, w, (x.shape[0], K, Hd, Wd), stride, pad)       # w read as the Conv2d weight [out = C, in = K]
    return y if b is None else y + b[None, :, None, None]


def deconv2d_dx(dy, w, stride, pad):
    """input gradient of deconv2d_fwd: the convolution of dy [B,K,Hd,Wd] with w [C,K,R,S]"""
    return conv2d_fwd(dy, w, None, stride, pad)


def deconv2d_dw(x, dy, R, S, stride, pad):
    """weight gradient [C,K,R,S] of deconv2d_fwd"""
    return conv2d_dw(dy, x, R, S, stride, pad)


def mask_a(R, S):
    """type-A mask of a MaskedConv2d [R,S]: the taps before the centre in raster order"""
    m = np.zeros((R, S))
    m.reshape(-1)[:(R // 2) * S + S // 2] = 1.0
    return m


def mask_b(R, S):
    """type-B mask: the type-A taps and the centre"""
    m = np.zeros((R, S))
    m.reshape(-1)[:(R // 2) * S + S // 2 + 1] = 1.0
    return m


def lrelu(v, slope):
    v = _f64(v)
    return np.where(v > 0, v, v * slope)


def dact(g, xact, slope):
    """derivative of the leaky ReLU applied to g, selected by the sign of the activation's OUTPUT xact (0.0 and -0.0: slope)"""
    g = _f64(g)
    return np.where(_f64(xact) > 0, g, g * slope)


def gdn_params(beta_p, gamma_p, beta_min=1e-6):
    """effective (beta, gamma) of the stored parameters: max(p, bound)^2 - 2^-36, bound = sqrt(beta_min + 2^-36) / 2^-18 (gdn.py)"""
    bb = np.sqrt(float(np.float32(beta_min)) + PEDESTAL)
    beta = np.maximum(_f64(beta_p), bb) ** 2 - PEDESTAL
    gamma = np.maximum(_f64(gamma_p), GAMMA_BOUND) ** 2 - PEDESTAL
    return beta, gamma


def gdn_norm(x, beta_p, gamma_p, beta_min=1e-6):
    """the denominator's square: norm[b,i,h,w] = beta[i] + sum_j gamma[i,j] x[b,j,h,w]^2"""
    beta, gamma = gdn_params(beta_p, gamma_p, beta_min)
    return np.einsum("ij,bjhw->bihw", gamma, _f64(x) ** 2) + beta[None, :, None, None]


def gdn_fwd(x, beta_p, gamma_p, inverse=0, beta_min=1e-6):
    """inverse 0: x / sqrt(norm) (GDN), 1: x * sqrt(norm) (IGDN), 2: norm itself (what the backward keeps)"""
    n = gdn_norm(x, beta_p, gamma_p, beta_min)
    if inverse == 2:
        return n
    return _f64(x) * np.sqrt(n) if inverse else _f64(x) / np.sqrt(n)


def gdn_gamma_contraction(g, x):
    """the gamma gradient's contraction: out[i,j] = sum_{b,h,w} g[b,i,h,w] * x[b,j,h,w]^2 (g: the dy-side operand)"""
    return np.einsum("bihw,bjhw->ij", _f64(g), _f64(x) ** 2)


def gdn_bwd(x, dy, beta_p, gamma_p, inverse=False, beta_min=1e-6):
    """-> (dx, dbeta, dgamma) with respect to the input and the STORED parameters; a parameter below its bound receives a
    gradient only when that gradient pushes it up (LowerBound: parametrizers.py / ops/bound_ops.py)"""
    x, dy = _f64(x), _f64(dy)
    beta, gamma = gdn_params(beta_p, gamma_p, beta_min)
    n = gdn_norm(x, beta_p, gamma_p, beta_min)
    g = 0.5 * dy * x / np.sqrt(n) if inverse else -0.5 * dy * x / (n * np.sqrt(n))
    u = dy * np.sqrt(n) if inverse else dy / np.sqrt(n)
    dx = u + 2.0 * x * np.einsum("ik,bihw->bkhw", gamma, g)
    dbeta_e, dgamma_e = g.sum(axis=(0, 2, 3)), gdn_gamma_contraction(g, x)

    def through_bound(p, bound, grad_e):
        p = _f64(p)
        gl = 2.0 * np.maximum(p, bound) * grad_e
        return np.where((p >= bound) | (gl < 0), gl, 0.0)
    bb = float(np.float32(np.sqrt(float(np.float32(beta_min)) + PEDESTAL)))
    return dx, through_bound(beta_p, bb, dbeta_e), through_bound(gamma_p, GAMMA_BOUND, dgamma_e)
