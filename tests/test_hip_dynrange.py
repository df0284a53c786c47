"""GPU: where the split-fp16 design is weakest -- ONE power-of-two scale per weight image / planes tensor -- judged PER CHANNEL.

Every fp32 value v travels as two fp16 numbers of v * 2^e with e chosen from the TENSOR's maximum (csrc/stem_common.h), so a
stored value carries a relative error of max(2^-22, 2^-25 * 2^-e / |v|): full 22 bits down to 2^-18 of the tensor's maximum,
one part in 10^5 at 2^-23 (1.2e-7 of the maximum), nothing below 2^-39.  The gates of the other test files (conftest.assert_close,
floor = 0.1) hold small elements to 1e-5 of the TENSOR's maximum; here every output channel is held to north_star's 1e-4 of ITS
OWN maximum (floor = 0), with output channel k of the weights scaled by 2^(-20 k / (K - 1)) -- a six-decade spread across the
channels of one layer, a thousand times what a trained layer shows -- and a GDN gamma whose off-diagonals are 1e-4 of its
diagonal (gdn.py:42-67), for every kernel family on the path: 192-column conv + GDN, first layer + GDN, general kernel (1x1,
strided, image-tile form), the transposed face, input gradients, both weight-gradient forms.  A second set of cases pushes the
spread to 2^-34 and checks the CONTRACT below the 22-bit range: an output channel is within 1e-4 of its own maximum or within
2^-36 of the tensor's maximum, whichever is larger -- the absolute floor the layout promises.  PLANES outputs (the copy of a
result handed to the next layer's kernel) are held to their own layout: 2^-22 relative or the grid of the second fp16 number
(2^-24 of the unit in the tensor's scale record, which comes from an upper bound of the outputs), whichever is larger.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))
import stem_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return functional


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().contiguous().numpy()


def spread(K, log2_span):
    """2^(-log2_span * k / (K - 1)), k = 0 .. K-1"""
    return (2.0 ** (-log2_span * np.arange(K) / max(K - 1, 1))).astype(np.float32)


def per_channel(a, ref, what, axis=1, span=20, rtol=1e-4, abs_floor=None):
    """every channel (index along `axis`) within rtol of ITS OWN maximum; for span > 20 also the layout's absolute floor
    (2^-36 of the tensor's maximum for results accumulated in fp32 from split operands; `abs_floor` for a planes tensor: the
    grid of its second fp16 number, 2^-24 of the unit its scale record states)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    red = tuple(i for i in range(ref.ndim) if i != axis)
    cmax = np.abs(ref).max(axis=red)
    err = np.abs(a - ref).max(axis=red)
    tol = rtol * cmax
    if abs_floor is not None:
        tol = np.maximum(tol, abs_floor)
        span = 99
    elif span > 20:
        tol = np.maximum(tol, 2.0 ** -36 * float(np.abs(ref).max()))
    worst = int(np.argmax(err / np.maximum(tol, 1e-300)))
    ratio = float((err / np.maximum(cmax, 1e-300)).max()) if span <= 20 else float((err / np.maximum(tol, 1e-300)).max())
    print(f"[per channel] {what}: worst {'err / own max' if span <= 20 else 'err / tolerance'} {ratio:.2e} at channel {worst} "
          f"(its max {cmax[worst]:.2e}, tensor max {np.abs(ref).max():.2e})")
    assert (err <= tol).all(), f"{what}: channel {worst}: err {err[worst]:.3e} > {tol[worst]:.3e} (own max {cmax[worst]:.3e})"


SPANS = [20, 34]


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("gdn", [False, True])
def test_192_column_kernel_per_channel(F, span, gdn):
    """g_a.2-like: 5x5 stride-2 conv 192 -> 192 (+ GDN with off-diagonals 1e-4 of the diagonal), fp32 and planes output"""
    B, C, H, W, K, R = 2, 192, 24, 20, 192, 5
    s = spread(K, span)
    x = rnd((B, C, H, W), 1, -2, 2)
    w = (rnd((K, C, R, R), 2) / np.sqrt(C * R * R)).astype(np.float32) * s[:, None, None, None]
    b = rnd((K,), 3, -0.1, 0.1) * s
    ref = orc.conv2d_fwd(x, w, b, 2, R // 2)
    kw = {}
    if gdn:
        beta = rnd((K,), 4, 0.5, 1.5)
        gamma = (1e-3 * rnd((K, K), 5, 0.5, 1.0) + 0.1 * np.eye(K, dtype=np.float32)).astype(np.float32)      # effective gamma (squared): off-diagonals ~1e-4 of the diagonal
        ref = orc.gdn_fwd(ref, beta, gamma)
        kw = dict(beta=dev(beta), gamma=dev(gamma))
    xp, wp = F.F16Planes.split(dev(x)), F.pack_weight_f16x2(dev(w))
    y = F.conv2d_f16x3_fwd(xp, wp, dev(b), K, R, R, 2, R // 2, **kw)
    per_channel(host(y), ref, f"192-column conv gdn={gdn} span 2^-{span}", span=span)
    yp = F.conv2d_f16x3_fwd(xp, wp, dev(b), K, R, R, 2, R // 2, planes_out=True, **kw)
    # a planes tensor has one scale too, taken from an upper BOUND of the outputs (K max|x| max|w| + max|b|: a few binades above the
    # real maximum): 2^-22 relative, or the grid of its second fp16 number -- whichever is larger
    per_channel(host(yp.merge()), ref, "... its planes output", abs_floor=2.0 ** -24 * yp.record()[0])


@pytest.mark.parametrize("span", SPANS)
def test_first_layer_gdn_per_channel(F, span):
    """g_a.0 + GDN (csrc/c4gdn_f16x3.hip): output channels of the 3 -> 192 convolution over six decades, thin gamma off-diagonals"""
    B, H, W, K, R = 2, 40, 56, 192, 5
    s = spread(K, span)
    x = rnd((B, 3, H, W), 11, 0, 1)
    w = (rnd((K, 3, R, R), 12) / np.sqrt(75)).astype(np.float32) * s[:, None, None, None]
    b = rnd((K,), 13, -0.1, 0.1) * s
    beta = rnd((K,), 14, 0.5, 1.5)
    gamma = (1e-3 * rnd((K, K), 15, 0.5, 1.0) + 0.1 * np.eye(K, dtype=np.float32)).astype(np.float32)
    ref = orc.gdn_fwd(orc.conv2d_fwd(x, w, b, 2, 2), beta, gamma)
    x4 = F.nchw3_to_nhwc4(dev(x))
    ast = F.c4gdn_stream(F.pack_weight(dev(w), F.PACK_CONV_FWD_C4), dev(gamma), K, R, R)
    y = F.conv2d_c4_gdn_f16x3(x4, ast, dev(b), dev(beta), K, R, R, 2, 2)
    per_channel(host(y), ref, f"first layer + GDN span 2^-{span}", span=span)


GEN = [  # name, B, C, H, W, K, R, stride
    ("EPM-like 1x1", 4, 576, 16, 16, 384, 1, 1),
    ("TPM-like 5x5 (image-tile form)", 4, 192, 16, 16, 256, 5, 1),
    ("HE.2-like strided 5x5", 4, 128, 16, 16, 128, 5, 2),
]


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("case", GEN, ids=[c[0] for c in GEN])
def test_general_kernel_per_channel(F, span, case):
    """forward + leaky ReLU (fp32 and planes) and -- stride 1 -- the input gradient with the layer's INPUT channels spread"""
    _, B, C, H, W, K, R, st = case
    s = spread(K, span)
    x = rnd((B, C, H, W), 21, -2, 2)
    w = (rnd((K, C, R, R), 22) / np.sqrt(C * R * R)).astype(np.float32) * s[:, None, None, None]
    b = rnd((K,), 23, -0.1, 0.1) * s
    ref = orc.conv2d_fwd(x, w, b, st, R // 2)
    ref = np.where(ref > 0, ref, ref * np.float32(0.01)).astype(np.float32)
    xp = F.F16Planes.split(dev(x))
    y, yp = F.conv2d_f16x3_gen(xp, F.pack_weight_f16x2_gen(dev(w)), dev(b), K, R, R, st, R // 2, epi=F.GEN_EPI_LRELU, want_planes=True)
    from spatiotemporalentropymodel_amd import _lib
    form = _lib.hip().stem_tuning_get(b"fx3_ran_form")            # the case's name is checked against the form that ran
    assert form == 3 if "image-tile form" in case[0] else form in (1, 2), (case[0], form)
    per_channel(host(y), ref, f"{case[0]} forward span 2^-{span}", span=span)
    per_channel(host(yp.merge()), ref, "... its planes output", abs_floor=2.0 ** -24 * yp.record()[0])
    if st == 1:        # input gradient: rows of the flipped image = the layer's input channels c; spread THOSE
        sc = spread(C, span)
        w2 = (rnd((K, C, R, R), 24) / np.sqrt(K * R * R)).astype(np.float32) * sc[None, :, None, None]
        dy = rnd((B, K, H, W), 25, -1, 1)
        dx_ref, _, _ = orc.conv2d_bwd(np.zeros((B, C, H, W), np.float32), w2, dy, 1, R // 2)
        dx, _ = F.conv2d_f16x3_gen(F.F16Planes.split(dev(dy)), F.pack_weight_f16x2_gen(dev(w2), flip=True), None, C, R, R, 1, R // 2)
        per_channel(host(dx), dx_ref, f"{case[0]} input gradient span 2^-{span}", span=span)


@pytest.mark.parametrize("span", SPANS)
def test_transposed_face_per_channel(F, span):
    """HD.2-like ConvTranspose2d forward over the four sub-pixel phases: output channels spread"""
    B, C, H, W, N, R = 4, 128, 8, 8, 160, 5
    s = spread(N, span)
    x = rnd((B, C, H, W), 31, -2, 2)
    w = (rnd((C, N, R, R), 32) / np.sqrt(C * R * R / 4)).astype(np.float32) * s[None, :, None, None]
    b = rnd((N,), 33, -0.1, 0.1) * s
    ref = orc.deconv2d_fwd(x, w, b, 2, 2, 1)
    y, yp = F.tconv2d_f16x3(F.F16Planes.split(dev(x)), F.pack_weight_f16x2_tconv(dev(w)), dev(b), N, R, want_planes=True)
    per_channel(host(y), ref, f"transposed face span 2^-{span}", span=span)
    per_channel(host(yp.merge()), ref, "... its planes output", abs_floor=2.0 ** -24 * yp.record()[0])


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("form", ["filter rows (stride 1, 16 x 16)", "per tap (stride 2)"])
def test_weight_gradients_per_channel(F, span, form):
    """dW[k] rows with the output-gradient channels k spread over six decades (an activation tensor with one scale), both
    weight-gradient forms; judged per output channel k of dW"""
    rows = form.startswith("filter")
    B, C, H, W, K, R = (4, 128, 16, 16, 160, 5)
    st = 1 if rows else 2
    s = spread(K, span)
    x = rnd((B, C, H, W), 41, -1, 1)
    dy = rnd((B, K, H // st, W // st), 42, -1, 1) * s[None, :, None, None]
    _, dw_ref, db_ref = orc.conv2d_bwd(x, np.zeros((K, C, R, R), np.float32), dy, st, R // 2, need_dx=False)
    xp, dyp = F.F16Planes.split(dev(x)), F.F16Planes.split(dev(dy))
    if rows:
        dw = torch.zeros(K, C, R, R, device="cuda")
        F.conv2d_wgrad_f16x3_into(xp, dyp, K, R, R, R // 2, dw, None, accumulate=False)
    else:
        splits, elems = F.wgrad_f16x3_strided_plan(xp.shape, K, R, R, 2, R // 2)
        dwp = torch.empty(elems, device="cuda")
        F.conv2d_wgrad_f16x3_strided(xp, dyp, K, R, R, 2, R // 2, dwp, splits)
        dw = dwp.view(splits, R * R, K, C).sum(0).permute(1, 2, 0).reshape(K, C, R, R)
    per_channel(host(dw), dw_ref, f"weight gradient, {form}, span 2^-{span}", axis=0, span=max(span, 21))     # dy is a planes tensor: one scale
