"""GPU tests at BASELINE.json's FULL sizes: the benchmarked kernels against the oracle on whole B=16 tensors (the C
oracle needs a few seconds per layer at these sizes), size-independent properties (linearity, adjoint identities
<Ax, y> = <x, A^T y> tying forward / dgrad / wgrad together, bit-reproducibility of a whole training step, batch
independence at the configs[4] workload), the 1088x1920 transforms against oracle crops and an encode -> decode round
trip of a 1080p-shaped latent (configs[3])."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import REPO, assert_close

sys.path.insert(0, os.path.join(REPO, "oracle"))
import stem_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu


def planes_match(yp, y):
    """planes copy vs fp32 copy: two fp16 numbers per value (|err| <= 2^-22 |y| + half a unit of the second plane's subnormal grid)"""
    inv, rec_max = yp.record()
    err = (yp.merge().double() - y.double()).abs()
    return bool((err <= y.double().abs() * 2.0 ** -22 + inv * 2.0 ** -25).all()) and rec_max == float(y.abs().max())



@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available()
    return functional


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def dot(a, b):
    return float((a.double() * b.double()).sum())


def test_analysis_conv_fullsize_linearity_and_spot_checks(F):
    """g_a.2 at the benchmark size: [16,192,128,128] -> [16,192,64,64], 5x5 stride 2 (120.8 GFLOP)."""
    torch.manual_seed(0)
    B, C, H, W, K = 16, 192, 128, 128, 192
    x1, x2 = cl(torch.randn(B, C, H, W, device="cuda")), cl(torch.randn(B, C, H, W, device="cuda"))
    w = torch.randn(K, C, 5, 5, device="cuda") * 0.02
    b = torch.randn(K, device="cuda")
    wp = F.pack_weight(w, F.PACK_CONV_FWD)
    y1, y2 = F.conv2d_fwd(x1, wp, b, K, 5, 5, 2, 2), F.conv2d_fwd(x2, wp, b, K, 5, 5, 2, 2)
    y3 = F.conv2d_fwd(cl(1.5 * x1 - 0.5 * x2), wp, b, K, 5, 5, 2, 2)
    lin = 1.5 * (y1 - b.view(1, -1, 1, 1)) - 0.5 * (y2 - b.view(1, -1, 1, 1)) + b.view(1, -1, 1, 1)
    err = float((y3 - lin).abs().max()) / float(lin.abs().max())
    assert err < 2e-5, err
    # single output pixels vs the oracle evaluated on the 5x5 input window (incl. image borders and last batch item)
    wn, bn = w.cpu().numpy(), b.cpu().numpy()
    for (bi, oy, ox) in [(0, 0, 0), (3, 17, 40), (15, 63, 63), (7, 0, 31), (9, 63, 0)]:
        win = torch.zeros(1, C, 5, 5)
        for r in range(5):
            for s in range(5):
                iy, ix = 2 * oy - 2 + r, 2 * ox - 2 + s
                if 0 <= iy < H and 0 <= ix < W:
                    win[0, :, r, s] = x1[bi, :, iy, ix].cpu()
        ref = orc.conv2d_fwd(win.numpy(), wn, bn, 1, 0)[0, :, 0, 0]
        assert_close(y1[bi, :, oy, ox].cpu().numpy(), ref, what=f"pixel {(bi, oy, ox)}", floor=0.1)


def test_fused_analysis_conv_gdn_fullsize_vs_oracle(F):
    """THE roofline kernel of bench.py at its benchmark shape -- igemm_kernel<128,192,...,FUSE>: g_a.2 (192->192, 5x5 s2,
    128^2 -> 64^2) with GDN g_a.3 fused into the epilogue, B=16 -- against the oracle's conv2d_fwd + gdn_fwd on the WHOLE
    tensor (it was only reached at B=1 / through properties)."""
    from spatiotemporalentropymodel_amd.weights import closed_form_tensor
    torch.manual_seed(21)
    B, C, H, W, K = 16, 192, 128, 128, 192
    x = cl(torch.randn(B, C, H, W, device="cuda"))
    w = closed_form_tensor("g_a.2.weight", (K, C, 5, 5))
    b = closed_form_tensor("g_a.2.bias", (K,))
    beta, gamma = closed_form_tensor("g_a.3.beta", (K,)), closed_form_tensor("g_a.3.gamma", (K, K))
    y = F.conv2d_gdn_fwd(x, F.pack_weight(w.cuda(), F.PACK_CONV_FWD), b.cuda(), beta.cuda(), gamma.cuda(), K, 5, 5, 2, 2)
    assert tuple(y.shape) == (B, K, 64, 64)
    ref = orc.gdn_fwd(orc.conv2d_fwd(x.cpu().contiguous().numpy(), w.numpy(), b.numpy(), 2, 2), beta.numpy(), gamma.numpy())
    assert_close(y.cpu().contiguous().numpy(), ref, what="fused g_a.2 + GDN at B=16", floor=0.1)
    # and the unfused pair gives the same numbers (same kernels the small-config goldens pin)
    y2 = F.gdn_fwd(F.conv2d_fwd(x, F.pack_weight(w.cuda(), F.PACK_CONV_FWD), b.cuda(), K, 5, 5, 2, 2), beta.cuda(), gamma.cuda())
    assert_close(y2.cpu().contiguous().numpy(), ref, what="g_a.2 then GDN at B=16", floor=0.1)


def test_f16x3_analysis_conv_gdn_fullsize_vs_oracle(F):
    """THE roofline kernel of bench.py since round 2 -- conv_f16x3_kernel<128,6>: g_a.2 (192->192, 5x5 s2, 128^2 -> 64^2) with
    GDN g_a.3 fused, B=16, planes in -> planes out, 128-pixel workgroups (the tile the library picks at this size) -- against
    the oracle's conv2d_fwd + gdn_fwd on the WHOLE tensor (the full-size check still exercised the fp32
    igemm kernel).  priors.py:424-425."""
    from spatiotemporalentropymodel_amd import _lib
    from spatiotemporalentropymodel_amd.weights import closed_form_tensor
    assert _lib.hip().stem_tuning_get(b"fx3_tile") == 0          # the library's own choice
    torch.manual_seed(21)
    B, C, H, W, K = 16, 192, 128, 128, 192
    x = cl(torch.randn(B, C, H, W, device="cuda"))
    w = closed_form_tensor("g_a.2.weight", (K, C, 5, 5))
    b = closed_form_tensor("g_a.2.bias", (K,))
    beta, gamma = closed_form_tensor("g_a.3.beta", (K,)), closed_form_tensor("g_a.3.gamma", (K, K))
    xp = F.F16Planes.split(x)
    assert planes_match(xp, x)
    yp = F.conv2d_f16x3_fwd(xp, F.pack_weight_f16x2(w.cuda()), b.cuda(), K, 5, 5, 2, 2, planes_out=True, beta=beta.cuda(), gamma=gamma.cuda())
    y = yp.merge()
    assert tuple(y.shape) == (B, K, 64, 64)
    ref = orc.gdn_fwd(orc.conv2d_fwd(x.cpu().contiguous().numpy(), w.numpy(), b.numpy(), 2, 2), beta.numpy(), gamma.numpy())
    assert_close(y.cpu().contiguous().numpy(), ref, what="f16x3 g_a.2 + GDN at B=16 (planes -> planes)", floor=0.1)
    # 64-pixel workgroups (the other tile of the same kernel) give the same tensor up to summation order
    with F.tuning(fx3_tile=64):
        y64 = F.conv2d_f16x3_fwd(xp, F.pack_weight_f16x2(w.cuda()), b.cuda(), K, 5, 5, 2, 2, beta=beta.cuda(), gamma=gamma.cuda())
    assert_close(y64.cpu().contiguous().numpy(), ref, what="f16x3 g_a.2 + GDN at B=16, 64-pixel tiles", floor=0.1)


def test_first_layer_gdn_fullsize_vs_oracle(F):
    """g_a.0 + GDN g_a.1 at the benchmark shape (B=16, 3 x 256^2 -> 192 x 128^2) on csrc/c4gdn_f16x3.hip, planes out (what the
    bench's analysis transform runs), whole tensor against the oracle.  priors.py:421-423."""
    from spatiotemporalentropymodel_amd.weights import closed_form_tensor
    torch.manual_seed(22)
    B, K = 16, 192
    x = torch.rand(B, 3, 256, 256, device="cuda")
    w, b = closed_form_tensor("g_a.0.weight", (K, 3, 5, 5)), closed_form_tensor("g_a.0.bias", (K,))
    beta, gamma = closed_form_tensor("g_a.1.beta", (K,)), closed_form_tensor("g_a.1.gamma", (K, K))
    assert F.c4gdn_supported(K, 5, 5)
    ast = F.c4gdn_stream(F.pack_weight(w.cuda(), F.PACK_CONV_FWD_C4), gamma.cuda(), K, 5, 5)
    yp = F.conv2d_c4_gdn_f16x3(F.nchw3_to_nhwc4(x), ast, b.cuda(), beta.cuda(), K, 5, 5, 2, 2, planes_out=True)
    y = yp.merge()
    assert tuple(y.shape) == (B, K, 128, 128)
    ref = orc.gdn_fwd(orc.conv2d_fwd(x.cpu().numpy(), w.numpy(), b.numpy(), 2, 2), beta.numpy(), gamma.numpy())
    assert_close(y.cpu().contiguous().numpy(), ref, what="g_a.0 + GDN at B=16 (c4gdn_f16x3, planes)", floor=0.1)


@pytest.mark.parametrize("name,shape", [("TPM.2", (16, 256, 16, 16, 320, 5)), ("TPM.4", (16, 320, 16, 16, 384, 5)), ("EPM.0", (16, 1152, 16, 16, 768, 1))])
def test_f16x3_training_kernels_fullsize_vs_oracle(F, name, shape):
    """The kernels the bench's P-frame step runs for the stride-1 STEM layers, at their B=16 shapes and with the planner's own
    split factors: conv_f16x3_gen_kernel forward (+ leaky ReLU, planes out) and input gradient (mirrored weight, x leaky-ReLU'),
    wgrad_f16x3_kernel with the bias gradient of the same pass -- whole tensors against the oracle
    (spatiotemporalpriors.py:807-838; VERDICT r2 weak #1: until now only route-vs-route agreement covered these plans)."""
    from spatiotemporalentropymodel_amd import _lib
    B, C, H, W, K, R = shape
    pad, sl = R // 2, 0.01
    assert _lib.hip().stem_tuning_get(b"fx3_split") == 0 and _lib.hip().stem_tuning_get(b"wg3_split") == 0
    torch.manual_seed(33)
    x = cl(torch.randn(B, C, H, W, device="cuda"))
    w = torch.randn(K, C, R, R, device="cuda") * (1.0 / (C * R * R) ** 0.5)
    b = torch.randn(K, device="cuda") * 0.1
    dy = cl(torch.randn(B, K, H, W, device="cuda"))
    xn, wn, bn, dyn = x.cpu().contiguous().numpy(), w.cpu().numpy(), b.cpu().numpy(), dy.cpu().contiguous().numpy()
    xp, dyp = F.F16Planes.split(x), F.F16Planes.split(dy)
    # forward
    y, yp = F.conv2d_f16x3_gen(xp, F.pack_weight_f16x2_gen(w), b, K, R, R, 1, pad, epi=F.GEN_EPI_LRELU, slope=sl, want_planes=True)
    ref = orc.conv2d_fwd(xn, wn, bn, 1, pad)
    ref = np.where(ref > 0, ref, ref * sl).astype(np.float32)
    assert_close(y.cpu().contiguous().numpy(), ref, what=f"{name} forward (f16x3 general kernel)", floor=0.1)
    assert planes_match(yp, y)
    # input gradient and weight / bias gradient
    rdx, rdw, rdb = orc.conv2d_bwd(xn, wn, dyn, 1, pad)
    rdx = np.where(xn > 0, rdx, rdx * sl).astype(np.float32)
    d, _ = F.conv2d_f16x3_gen(dyp, F.pack_weight_f16x2_gen(w, flip=True), None, C, R, R, 1, pad, epi=F.GEN_EPI_DACT, slope=sl, z=x)
    assert_close(d.cpu().contiguous().numpy(), rdx, what=f"{name} input gradient (f16x3 general kernel)", floor=0.1)
    splits, elems = F.wgrad_f16x3_plan(x.shape, K, R, R, pad)
    dwp = torch.empty(elems, device="cuda")
    db = torch.full((K,), float("nan"), device="cuda")
    F.conv2d_wgrad_f16x3(xp, dyp, K, R, R, pad, dwp, splits, db=db)
    dw = dwp.view(splits, R * R, K, C).sum(0).permute(1, 2, 0).reshape(K, C, R, R)
    print(f"{name}: wgrad splits {splits}")
    assert_close(dw.cpu().numpy(), rdw, what=f"{name} weight gradient (wgrad_f16x3)", floor=0.1)
    assert_close(db.cpu().numpy(), rdb, what=f"{name} bias gradient (wgrad_f16x3 pass)", floor=0.1)


@pytest.mark.parametrize("name,shape", [("TPM.2", (16, 256, 16, 16, 320, 5, 1, 2)), ("HE.2", (16, 256, 16, 16, 256, 5, 2, 2)),
                                        ("EPM.0", (16, 1152, 16, 16, 768, 1, 1, 0))])
def test_conv_gradients_fullsize_vs_oracle(F, name, shape):
    """dgrad, wgrad (every tap) and the bias gradient of the STEM layers at their B=16 training shapes against the
    oracle's conv2d_bwd on the full tensors -- values, not only the adjoint identities."""
    B, C, H, W, K, R, st, pd = shape
    torch.manual_seed(31)
    x = cl(torch.randn(B, C, H, W, device="cuda"))
    w = torch.randn(K, C, R, R, device="cuda") * 0.05
    Ho, Wo = F.conv_out_hw(H, W, R, R, st, pd)
    dy = cl(torch.randn(B, K, Ho, Wo, device="cuda"))
    dx = F.conv2d_dgrad(dy, F.pack_weight(w, F.PACK_CONV_DGRAD), x.shape, K, R, R, st, pd)
    dw, db = F.conv2d_wgrad(x, dy, K, R, R, st, pd)
    rdx, rdw, rdb = orc.conv2d_bwd(x.cpu().contiguous().numpy(), w.cpu().numpy(), dy.cpu().contiguous().numpy(), st, pd)
    assert_close(dx.cpu().contiguous().numpy(), rdx, what=f"{name} dgrad", floor=0.1)
    assert_close(dw.cpu().numpy(), rdw, what=f"{name} wgrad", floor=0.1)
    assert_close(db.cpu().numpy(), rdb, what=f"{name} bias gradient", floor=0.1)


def test_deconv_gradients_fullsize_vs_oracle(F):
    """HD.2 (ConvTranspose2d 256->256, 5x5 s2, 8^2 -> 16^2) at B=16: forward, dgrad, wgrad, bias gradient vs the oracle."""
    B, C, H, W, K = 16, 256, 8, 8, 256
    torch.manual_seed(32)
    x = cl(torch.randn(B, C, H, W, device="cuda"))
    w = torch.randn(C, K, 5, 5, device="cuda") * 0.05
    bias = torch.randn(K, device="cuda")
    y = F.deconv2d_fwd(x, F.pack_weight(w, F.PACK_DECONV_FWD), bias, K, 5, 5, 2, 2, 1)
    xn, wn = x.cpu().contiguous().numpy(), w.cpu().numpy()
    assert_close(y.cpu().contiguous().numpy(), orc.deconv2d_fwd(xn, wn, bias.cpu().numpy(), 2, 2, 1), what="HD.2 forward", floor=0.1)
    dy = cl(torch.randn_like(y))
    dx = F.deconv2d_dgrad(dy, F.pack_weight(w, F.PACK_DECONV_DGRAD), x.shape, K, 5, 5, 2, 2, 1)
    dw, db = F.deconv2d_wgrad(x, dy, K, 5, 5, 2, 2, 1)
    rdx, rdw, rdb = orc.deconv2d_bwd(xn, wn, dy.cpu().contiguous().numpy(), 2, 2, 1)
    assert_close(dx.cpu().contiguous().numpy(), rdx, what="HD.2 dgrad", floor=0.1)
    assert_close(dw.cpu().numpy(), rdw, what="HD.2 wgrad", floor=0.1)
    assert_close(db.cpu().numpy(), rdb, what="HD.2 bias gradient", floor=0.1)


@pytest.mark.parametrize("shape", [(16, 256, 16, 16, 320, 5, 1, 2), (16, 256, 16, 16, 256, 5, 2, 2), (16, 1152, 16, 16, 768, 1, 1, 0)])
def test_adjoint_identities_fullsize(F, shape):
    """<conv(x), dy> = <x, dgrad(dy)> = <w, wgrad(x, dy)> (bias-free) at B=16 STEM layer sizes: TPM.2, HE.2, EPM.0."""
    B, C, H, W, K, R, st, pd = shape
    torch.manual_seed(1)
    x = cl(torch.randn(B, C, H, W, device="cuda"))
    w = torch.randn(K, C, R, R, device="cuda") * 0.05
    y = F.conv2d_fwd(x, F.pack_weight(w, F.PACK_CONV_FWD), None, K, R, R, st, pd)
    dy = cl(torch.randn_like(y))
    dx = F.conv2d_dgrad(dy, F.pack_weight(w, F.PACK_CONV_DGRAD), x.shape, K, R, R, st, pd)
    dw, db = F.conv2d_wgrad(x, dy, K, R, R, st, pd)
    s_fwd, s_dgrad, s_wgrad = dot(y, dy), dot(x, dx), dot(w, dw)
    scale = float(y.double().norm() * dy.double().norm())
    assert abs(s_fwd - s_dgrad) < 1e-5 * scale and abs(s_fwd - s_wgrad) < 1e-5 * scale, (s_fwd, s_dgrad, s_wgrad)
    assert_close(db.cpu().numpy(), dy.double().sum((0, 2, 3)).float().cpu().numpy(), what="bias gradient", floor=0.1)


def test_deconv_adjoint_fullsize(F):
    B, C, H, W, K = 16, 256, 8, 8, 256                      # HD.2
    torch.manual_seed(2)
    x = cl(torch.randn(B, C, H, W, device="cuda"))
    w = torch.randn(C, K, 5, 5, device="cuda") * 0.05
    y = F.deconv2d_fwd(x, F.pack_weight(w, F.PACK_DECONV_FWD), None, K, 5, 5, 2, 2, 1)
    assert tuple(y.shape) == (B, K, 16, 16)
    dy = cl(torch.randn_like(y))
    dx = F.deconv2d_dgrad(dy, F.pack_weight(w, F.PACK_DECONV_DGRAD), x.shape, K, 5, 5, 2, 2, 1)
    dw, _ = F.deconv2d_wgrad(x, dy, K, 5, 5, 2, 2, 1)
    s = dot(y, dy)
    scale = float(y.double().norm() * dy.double().norm())
    assert abs(s - dot(x, dx)) < 1e-5 * scale and abs(s - dot(w, dw)) < 1e-5 * scale


def test_config2_training_step_is_bit_reproducible():
    """configs[1] shapes (B=16, N=M=192, ebc=256): two runs of the same P-frame step from the same state give
    bit-identical gradients and parameters (no float atomics anywhere on the gradient path)."""
    from spatiotemporalentropymodel_amd.losses import EMLoss
    from spatiotemporalentropymodel_amd.optim import configure_optimizers
    from spatiotemporalentropymodel_amd.selfcheck import p_frame_step
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    from spatiotemporalentropymodel_amd.zoo import models
    dev = torch.device("cuda:0")
    outs = []
    for _ in range(2):
        torch.manual_seed(7)
        imodel = models["mbt2018"](quality=4).to(dev).eval()
        stem = SpatioTemporalPriorModel_Res().to(dev).train()
        opt, aux = configure_optimizers(stem, types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3))
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        frames = [torch.rand(16, 3, 256, 256, device=dev, generator=g) for _ in range(2)]
        with torch.no_grad():
            _, y_cond = imodel.getY(frames[0])
        out, oc, auxl, gn = p_frame_step(imodel, stem, EMLoss(), opt, aux, frames[1], y_cond)
        torch.cuda.synchronize()
        outs.append((opt.flat.grad.clone(), opt.flat.data.clone(), float(oc["loss"].detach()), float(gn), out["y_hat"].clone()))
    assert torch.equal(outs[0][0], outs[1][0]), "gradients differ between two identical runs"
    assert torch.equal(outs[0][1], outs[1][1]), "parameters differ between two identical runs"
    assert torch.equal(outs[0][4], outs[1][4])
    assert abs(outs[0][2] - outs[1][2]) <= 1e-12 * abs(outs[0][2]) and np.isfinite(outs[0][2]) and outs[0][3] > 0
    assert tuple(outs[0][4].shape) == (16, 192, 16, 16)


def test_1080p_latent_roundtrip_config4():
    """configs[3]: 1920x1080 frame padded to 1088 -> y [1,192,68,120], z [1,256,17,30]: compress -> decompress."""
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_
    dev = torch.device("cuda:0")
    m = SpatioTemporalPriorModel_Res()
    closed_form_fill_(m)
    m = m.to(dev).eval()
    m.update(force=True)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    y_cond = torch.randn(1, 192, 68, 120, device=dev, generator=g) * 3
    y_cur = y_cond + torch.randn(1, 192, 68, 120, device=dev, generator=g) * 2
    with torch.no_grad():
        enc = m.compress(y_cur, y_cond)
        assert tuple(enc["shape"]) == (17, 30)
        enc2 = m.compress(y_cur, y_cond)
        assert enc2["strings"][0][0] == enc["strings"][0][0] and enc2["strings"][1][0] == enc["strings"][1][0]
        y_hat = m.decompress(enc["strings"], enc["shape"], y_cond)["y_hat"]
    assert tuple(y_hat.shape) == (1, 192, 68, 120)
    # y_hat = round(res - mu) + mu + y_cond  =>  within half a quantisation step of y_cur everywhere
    err = float((y_hat - y_cur).abs().max())
    assert err <= 0.5 + 1e-4, err
    bpp = 8 * (len(enc["strings"][0][0]) + len(enc["strings"][1][0])) / (1088 * 1920)
    assert 0 < bpp < 24


def test_roi_gop_iteration_is_bit_reproducible():
    """configs[4] shapes at reduced batch (B=2, 3 frames of 256x256): two GOP iterations from the same state give
    bit-identical accumulated gradients and stepped parameters -- the weight-gradient side stream, the shared
    geometry-keyed workspaces and the accumulate-in-place kernels introduce no ordering dependence."""
    from spatiotemporalentropymodel_amd.losses import PixelwiseRateDistortionLoss
    from spatiotemporalentropymodel_amd.models import stem_roi, stem_roi_i
    from spatiotemporalentropymodel_amd.optim import configure_optimizers
    from spatiotemporalentropymodel_amd.selfcheck import roi_gop_step
    dev = torch.device("cuda:0")
    res = []
    for _ in range(2):
        torch.manual_seed(5)
        imodel, pmodel = stem_roi_i().to(dev).train(), stem_roi().to(dev).train()
        for i, m in enumerate((imodel, pmodel)):
            m.entropy_bottleneck.noise_seed = m.gaussian_conditional.noise_seed = 77 + i
        args = types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3)
        opts = configure_optimizers(imodel, args, max_norm=None) + configure_optimizers(pmodel, args, max_norm=None)
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        frames = [torch.rand(2, 3, 256, 256, device=dev, generator=g) for _ in range(3)]
        qmap = torch.rand(2, 1, 256, 256, device=dev, generator=g)
        log = roi_gop_step(imodel, pmodel, PixelwiseRateDistortionLoss(), opts, frames, qmap, 1.0)
        torch.cuda.synchronize()
        res.append(([o.flat.grad.clone() for o in opts], [o.flat.data.clone() for o in opts], [float(l[1]) for l in log]))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b), "accumulated gradients differ between two identical GOP iterations"
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b), "parameters differ between two identical GOP iterations"
    assert res[0][2] == res[1][2] and all(np.isfinite(a) and a > 0 for a in res[0][2])      # clip norms: no atomics either


def test_transforms_1080p_vs_oracle_crops_config4():
    """configs[3]: getY / getX at the eval geometry -- a 1920x1080 frame padded to 1088x1920 (stem/evalSTEM.py:96-109),
    y [1,192,68,120] -- against the oracle's g_a / g_s evaluated on 256x256 crops (16x16 latents).  A crop reproduces
    the full-image result wherever the receptive field stays inside it (or where the crop edge IS the image edge, so the
    zero padding coincides): 4 px of margin in latent units for g_a, 64 px in pixel units for g_s."""
    from spatiotemporalentropymodel_amd.selfcheck import build_models
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    dev = torch.device("cuda:0")
    imodel, _ = build_models(64, 96, 192, 192, dev)
    isd = {k: v.detach().cpu().numpy() for k, v in imodel.state_dict().items() if v.dtype == torch.float32}
    Hp, Wp = 1088, 1920
    big = smooth_frames("1080p", 1, 1, 2048)[0][:, :, :Hp, :Wp].contiguous()       # [1,3,1088,1920] in [0,1]
    with torch.no_grad():
        y, _ = imodel.getY(big.to(dev))
    assert tuple(y.shape) == (1, 192, 68, 120)
    yh = y.cpu().contiguous().numpy()
    M = 4
    for (py, px) in [(0, 0), (Hp - 256, Wp - 256), (416, 832), (0, 1008), (592, 0)]:       # multiples of 16 (stride phase)
        ref = orc.g_a(isd, big[:, :, py:py + 256, px:px + 256].contiguous().numpy())             # [1,192,16,16]
        ly, lx = py // 16, px // 16
        y0, y1 = (0 if py == 0 else M), (16 if py + 256 == Hp else 16 - M)
        x0, x1 = (0 if px == 0 else M), (16 if px + 256 == Wp else 16 - M)
        assert_close(yh[:, :, ly + y0:ly + y1, lx + x0:lx + x1], ref[:, :, y0:y1, x0:x1], what=f"getY crop at {(py, px)}", floor=0.1)
    # synthesis on the quantised latents of that frame -> [1,3,1088,1920]; the oracle's g_s without its final clip
    yl = y.round()
    with torch.no_grad():
        pre = imodel.g_s(yl)                                  # NHWC, before the clamp
        xh = imodel.getX(yl)
    assert tuple(xh.shape) == (1, 3, Hp, Wp) and xh.is_contiguous()
    # getX == clamp(g_s) exactly (the clamp is fused into the NHWC -> NCHW pass)
    assert torch.equal(xh, pre.contiguous(memory_format=torch.contiguous_format).clamp(0, 1))
    pn, yn = pre.cpu().contiguous().numpy(), yl.cpu().contiguous().numpy()

    def g_s_noclip(lat):
        h = lat
        for i in range(4):
            h = orc.deconv2d_fwd(h, isd[f"g_s.{2 * i}.weight"], isd[f"g_s.{2 * i}.bias"], 2, 2, 1)
            if i < 3:
                h = orc.gdn_fwd(h, isd[f"g_s.{2 * i + 1}.beta"], isd[f"g_s.{2 * i + 1}.gamma"], inverse=True)
        return h

    P = 64
    for (ly, lx) in [(0, 0), (68 - 16, 120 - 16), (20, 50), (0, 70), (40, 0)]:
        ref = g_s_noclip(np.ascontiguousarray(yn[:, :, ly:ly + 16, lx:lx + 16]))                 # [1,3,256,256]
        y0, y1 = (0 if ly == 0 else P), (256 if ly + 16 == 68 else 256 - P)
        x0, x1 = (0 if lx == 0 else P), (256 if lx + 16 == 120 else 256 - P)
        got = pn[:, :, ly * 16 + y0:ly * 16 + y1, lx * 16 + x0:lx * 16 + x1]
        assert_close(got, ref[:, :, y0:y1, x0:x1], what=f"g_s crop at latent {(ly, lx)}", floor=0.1)
        np.testing.assert_array_equal(np.clip(ref, 0, 1), orc.g_s(isd, np.ascontiguousarray(yn[:, :, ly:ly + 16, lx:lx + 16])))


def test_variable_rate_workload_config5_properties():
    """configs[4] at its stated workload: the variable-rate pair (stem_roi_i, stem_roi) on B=16 samples of 256x256 whose
    quality maps are uniform at the four levels {0.30, 0.45, 0.55, 0.70}, four samples per level (the four lambda points
    of stem_roi/eval_stem_roi.py:368-376 in one batch; lambda = quality2lambda, utils.py:97-101).  The reference pins these
    models at B=1 (test_hip_roi.py goldens); here the B=16 run is tied to them through batch independence: every level's
    4-sample group run on its own gives the same reconstructions / likelihoods, the batch loss is the mean of the group
    losses, and the batch gradient the mean of the group gradients (the criterion averages over the batch)."""
    from dp_worker import SlicedNoise
    from spatiotemporalentropymodel_amd.losses import PixelwiseRateDistortionLoss, quality2lambda
    from spatiotemporalentropymodel_amd.models import stem_roi, stem_roi_i
    from spatiotemporalentropymodel_amd.weights import closed_form_fill_scaled_, smooth_frames
    dev = torch.device("cuda:0")
    B, levels = 16, (0.30, 0.45, 0.55, 0.70)
    imodel = closed_form_fill_scaled_(stem_roi_i(), "stem_roi_i", 0.7).to(dev).train()
    pmodel = closed_form_fill_scaled_(stem_roi(), "stem_roi", 0.7).to(dev).train()
    frames = [f.to(dev) for f in smooth_frames("cfg5", B, 2, 256)]
    qmap = torch.cat([torch.full((4, 1, 256, 256), q) for q in levels]).to(dev)
    lam = quality2lambda(qmap)
    for q, row in zip(levels, lam[::4, 0, 0, 0].tolist()):
        assert abs(row - 0.002 * np.exp(3.4409 * q)) < 1e-6 * row          # fp32 exp
    crit = PixelwiseRateDistortionLoss()

    def run(lo, hi):
        n, world, rank = hi - lo, B // (hi - lo), lo // (hi - lo)
        for m, tag in ((imodel, "i"), (pmodel, "p")):
            m.zero_grad(set_to_none=True)
            m.entropy_bottleneck.noise_source = SlicedNoise(f"cfg5_{tag}_eb", rank, world, n, batch_last=True)
            m.gaussian_conditional.noise_source = SlicedNoise(f"cfg5_{tag}_gc", rank, world, n)
        out_i = imodel(frames[0][lo:hi], qmap[lo:hi])
        out_p = pmodel(frames[1][lo:hi], out_i["x_hat"], qmap[lo:hi])             # x_hat NOT detached (train_stem_roi.py:548)
        li = crit(out_i, frames[0][lo:hi], lam[lo:hi])
        lp = crit(out_p, frames[1][lo:hi], lam[lo:hi])
        (li["loss"] + lp["loss"]).backward()
        grads = {f"{t}.{k}": p.grad.detach().clone() for t, m in (("i", imodel), ("p", pmodel)) for k, p in m.named_parameters()
                 if p.grad is not None}
        return out_i, out_p, float(li["loss"]) + float(lp["loss"]), float(lp["bpp_loss"]), grads

    oi, op, loss16, _, g16 = run(0, B)
    assert tuple(op["x_hat"].shape) == (B, 3, 256, 256) and np.isfinite(loss16)
    # ---- the B=16 run against the CPU oracle (this workload was tied to the goldens through properties only): one
    # sample per quality level through oracle/stem_oracle.py:stem_roi_forward -- I frame, then the P frame conditioned on the
    # ORACLE's own reconstruction -- with the very noise rows the batch run drew; x_hat, both likelihoods and the sample's loss
    isd = {k: v.detach().cpu().numpy() for k, v in imodel.state_dict().items()}
    psd = {k: v.detach().cpu().numpy() for k, v in pmodel.state_dict().items()}
    from spatiotemporalentropymodel_amd.weights import closed_form_input

    def noise_rows(tag, b, zc, zhw):
        zfull = closed_form_input(f"noise:cfg5_{tag}_eb:0", (zc, 1, zhw * zhw * B), -0.5, 0.5).reshape(zc, zhw * zhw, B)
        yfull = closed_form_input(f"noise:cfg5_{tag}_gc:0", (B, 192, 16, 16), -0.5, 0.5)
        return {"z": zfull[:, :, b].reshape(1, zc, zhw, zhw).numpy().copy(), "y": yfull[b:b + 1].numpy().copy()}

    def sample_loss(o, target, lam_b):
        bpp = orc.rate_bpp(o["lik_y"], 256 * 256) + orc.rate_bpp(o["lik_z"], 256 * 256)
        mse = float(np.mean(lam_b.astype(np.float64) * (o["x_hat"].astype(np.float64) - target) ** 2))
        return bpp + 255 ** 2 * mse

    zc_i, zc_p = oi["likelihoods"]["z"].shape[1], op["likelihoods"]["z"].shape[1]
    zhw = oi["likelihoods"]["z"].shape[2]
    for b in (0, 4, 8, 12):
        f0, f1 = frames[0][b:b + 1].cpu().numpy(), frames[1][b:b + 1].cpu().numpy()
        qb, lb = qmap[b:b + 1].cpu().numpy(), lam[b:b + 1].cpu().numpy()
        ro_i = orc.stem_roi_forward(isd, f0, None, qb, noise_rows("i", b, zc_i, zhw), temporal=False)
        ro_p = orc.stem_roi_forward(psd, f1, ro_i["x_hat"], qb, noise_rows("p", b, zc_p, zhw), temporal=True)
        for tag, ro, go in (("I", ro_i, oi), ("P", ro_p, op)):
            assert_close(go["x_hat"][b:b + 1].detach().cpu().numpy(), ro["x_hat"], 1e-4, what=f"sample {b} {tag} x_hat vs oracle", floor=0.1)
            assert_close(go["likelihoods"]["y"][b:b + 1].detach().cpu().contiguous().numpy(), ro["lik_y"], 1e-4, atol=1e-9,
                         what=f"sample {b} {tag} lik_y vs oracle", floor=0.1)
            assert_close(go["likelihoods"]["z"][b:b + 1].detach().cpu().contiguous().numpy(), ro["lik_z"], 1e-4, atol=1e-9,
                         what=f"sample {b} {tag} lik_z vs oracle", floor=0.1)
        # the batch criterion is the mean over samples: a sample's loss from the GPU tensors against the oracle's
        for tag, ro, go, tgt in (("I", ro_i, oi, f0), ("P", ro_p, op, f1)):
            g_one = {"x_hat": go["x_hat"][b:b + 1].detach().cpu().numpy(), "lik_y": go["likelihoods"]["y"][b:b + 1].detach().cpu().contiguous().numpy(),
                     "lik_z": go["likelihoods"]["z"][b:b + 1].detach().cpu().contiguous().numpy()}
            lg, lo_ = sample_loss(g_one, tgt, lb), sample_loss(ro, tgt, lb)
            assert abs(lg - lo_) <= 1e-4 * abs(lo_), (b, tag, lg, lo_)
    acc, losses, bpps = None, [], []
    for gi in range(4):
        gi_i, gi_p, lg, bpp, gg = run(4 * gi, 4 * gi + 4)
        sl = slice(4 * gi, 4 * gi + 4)
        # B=16 and B=4 pick different tile / split-K plans: same values up to fp32 summation order through ~60 layers
        assert_close(gi_p["x_hat"].detach().cpu().numpy(), op["x_hat"][sl].detach().cpu().numpy(), 1e-4, what=f"level {gi} x_hat", floor=0.1)
        assert_close(gi_p["likelihoods"]["y"].detach().cpu().contiguous().numpy(), op["likelihoods"]["y"][sl].detach().cpu().contiguous().numpy(),
                     1e-4, atol=1e-9, what=f"level {gi} lik_y", floor=0.1)
        losses.append(lg)
        bpps.append(bpp)
        acc = gg if acc is None else {k: acc[k] + v for k, v in gg.items()}
    assert abs(np.mean(losses) - loss16) <= 1e-5 * abs(loss16), (losses, loss16)
    assert len(g16) > 500
    # gradients: same criterion as test_hip_roi.py::test_roi_batch_and_nonsquare_consistency (a leaky-ReLU pre-activation
    # within fp32 noise of 0 may flip sides when the batch size changes the tile / split-K plan; the few tensors below
    # such an element move by up to ~1e-3 of their cancelling sums, everything else agrees to fp32 rounding)
    errs = []
    for k, v in g16.items():
        ref = (acc[k] / 4).double()
        scale = float(ref.abs().max()) or 1.0
        errs.append((float((v.double() - ref).abs().max()) / scale, k))
    errs.sort(reverse=True)
    loose = [e for e in errs if e[0] > 1e-4]
    print(f"configs[4] B=16, 4 lambda levels: batch gradient vs mean of per-level gradients over {len(errs)} tensors: worst err / max = "
          f"{errs[0][0]:.2e} ({errs[0][1]}), {len(loose)} above 1e-4, median {errs[len(errs) // 2][0]:.1e}; per-level P-frame bpp "
          f"{['%.3f' % b for b in bpps]}")
    # measured on MI355X: median 2e-5, 169 of 540 tensors above 1e-4, worst 7.7e-3 (hyper-path SFT MLPs, whose inputs are
    # CONSTANT over space for these uniform quality maps: their gradients are sums over all pixels of terms that cancel)
    # the property bound was 2e-2; with the forward tied to the oracle above, the gradient identity is held to 1e-2
    # on the worst tensor (measured 7.7e-3 on the spatially constant SFT MLPs) and to 5e-3 on all but eight tensors
    assert errs[len(errs) // 2][0] <= 1e-4 and errs[0][0] < 1e-2 and errs[8][0] < 5e-3 and len(loose) <= 0.4 * len(errs), errs[:10]


def test_first_launch_on_fresh_workspaces_is_reproducible():
    """The split-K arrival protocol (partials of a tile written by workgroups on different XCDs, a ticket per workgroup, the last
    arriver sums them: csrc/stem_common.h `splitk_last_arriver`) on its hardest case: the FIRST launches after the workspaces
    were (re)allocated -- round 4's 16-byte-store form let the ticket overtake the data exactly there and the last arriver
    summed the allocation's zeros.  Eight fresh big models (fresh engines, workspaces, counters) at the bench geometry: every
    run's training forward gives the same TPM.0 output as a recomputation afterwards, and all runs give the same tensors."""
    import types
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    from spatiotemporalentropymodel_amd.optim import configure_optimizers
    dev = torch.device("cuda:0")
    runs = []
    for r in range(8):
        torch.manual_seed(7)
        torch.cuda.empty_cache()                                   # the next run's workspaces come from fresh allocations
        stem = SpatioTemporalPriorModel_Res().to(dev).train()
        configure_optimizers(stem, types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3))
        for m in (stem.entropy_bottleneck, stem.gaussian_conditional):
            m.noise_seed = 99
        g = torch.Generator(device=dev).manual_seed(11)
        y_cur = torch.randn(16, 192, 16, 16, device=dev, generator=g) * 3
        y_cond = y_cur + torch.rand(16, 192, 16, 16, device=dev, generator=g) - 0.5
        eng = stem.engine()
        y_hat, lik_y, lik_z, k = eng.forward(y_cur, y_cond, True)
        torch.cuda.synchronize()
        again = eng.TPM[0].forward(k["acts"]["yd"], F.ACT_LRELU, planes=True).x      # from the very planes the forward read
        torch.cuda.synchronize()
        assert torch.equal(again, k["tp0"]), f"run {r}: TPM.0 inside the forward differs from its recomputation"
        runs.append({n: k[n].clone() for n in ("he0", "he2", "hd0", "hd2", "tp0", "tp2", "e0", "e2", "gp") if isinstance(k.get(n), torch.Tensor)}
                    | {"lik_y": lik_y.clone(), "y_hat": y_hat.clone()})
        del stem, eng, k
    for r in range(1, len(runs)):
        diff = [n for n in runs[0] if not torch.equal(runs[0][n], runs[r][n])]
        assert not diff, (r, diff)
