"""GPU: the 192-column kernel conv_f16x3_kernel<BM, DEPTH, MS> (csrc/conv_f16x3.hip) behind stem_conv2d_f16x3_fwd (bias, fused
GDN) and stem_conv2d_f16x3_fwd_act (leaky ReLU; with the flipped pack the input gradient of the layer-wise models) -- under EVERY
one of its six instantiations, forced through F.tuning(fx3_tile = 64 | 128, fx3_depth = 2 | 3, fx3_mfma = 16 | 32) and read back
through stem_tuning_get("fx3_col_ran_tile" | "fx3_col_ran_depth" | "fx3_col_ran_mfma"), which must equal the restatement
fx3_col_cases.col_instantiation (fx3_mfma = 16 with the two-stage loop runs the 32-row shape: asserted).  Shapes and the host
arithmetic: tests/fx3_col_cases.py, pinned on the CPU by tests/test_fx3_col_plan_abi.py: chunk counts 1 .. 7 (prologue clamp, pair
loop + tail, stage rotation mod 3) from C in {32, 64, 128} with 1x1, 1x3, 1x5 and 1x7 windows, the 5x5 stride-2 192 -> 192 layer at
20 x 28, N in {192, 100, 96, 64, 33}, M < 64, M tails on both tiles, tiles that straddle rows and images, a grid of 35 / 18
workgroups (the XCD remap's remainder branch), pad 0 and pad > R / 2, strides 1 .. 3, output into a channel slice (ldy = N + 12).

Gate: every output channel within 1e-4 of ITS OWN maximum against float64 (tests/conv_ref.py), no floor
(test_hip_f16x3_forms.per_channel); random inputs carry output channel k at the scale 2^(-20 k / (N - 1)) under one scale record.
Planes outputs are held to their own layout (1e-4 of the channel's maximum or the grid of the second fp16 number) and to
test_hip_f16x3.planes_match against the fp32 copy of the same launch.

Exact relations asserted on top:
  * integer inputs in [-8, 8], integer bias, slope 0.5: the convolution without GDN EQUALS float64, hence all six forms agree to
    the bit (C R S 64 < 2^24: every partial sum is an integer below 2^24 times one power of two); with the fused GDN the forms
    are not compared bit for bit (the 16-row shape sums the second contraction in another order);
  * systematic residuals (wg3_cases.resid) on activations and weights: each cross product carries more than the gate of EVERY
    output (shown on the CPU), so a form that drops one fails;
  * the same launch twice is bit-identical, fp32, planes and scale records byte for byte;
  * sentinels outside the output's channel slice are untouched; no NaN;
  * fp32 output with a record but no planes: inv = 1, one slot per workgroup, their maximum is max|y|, nothing behind them;
  * GDN of a batch whose second image is zero, without bias: exact zeros there (whole tiles have vm = 0), finite record;
  * GDN of pixels that step down to 2^-16 of their tile's maximum: held PER ELEMENT to the bound the kernel's own statement gives
    (csrc/conv_f16x3.hip "t = v 2^ev with |t| < 2^7, t^2 < 2^14"): the squares are scaled by the TILE's maximum vm (vm 2^ev in
    [2^6, 2^7)) and stored as two fp16 numbers, which miss up to d(t^2) = max(2^-22 t^2, 2^-25) (half a unit of the subnormal grid
    2^-24).  With E_i = 1/2 sum_j gamma'_ij d(t_j^2) / (norm_i 2^(2 ev)) the output may be off by
        |y_i - ref_i| <= 2^-20 l1_i / sqrt(norm_i) + |ref_i| (2 E_i + 2^-18)
    (l1 = sum |x| |w| of the convolution: three split errors and one accumulation error of 2^-22 each; the factor 2 on E is the
    margin for the second contraction's own products and accumulation; 2^-18 covers the convolution's error inside the norm, the
    approximate reciprocal square root and the final rounding).  Consequence, written here and in DESIGN.md 3/4: a pixel whose
    amplitude is rho of its tile's maximum has its norm off by up to 2^-25 / t^2 with t >= 2^6 rho, its output by half of that,
    2^-38 / rho^2 -- 1e-4 per element is no longer met below rho = 2^-12.4 = 1.9e-4 of the tile's maximum (2^-13.4 where the
    maximum sits at the top of its binade); at 2^-16 the bound is 2^-6.  rho is the amplitude of the VALUES: in this file's case
    (pixels at steps 2^0 .. 2^-16 whose values lie below their step) E passes 1e-4 between the steps 2^-10 and 2^-12.

Exclusions -- refused by the library with an error (asserted), nothing else is left out:
  * planes output of the N = 100 and N = 33 shapes ("planes output needs N % 32 == 0"): fp32 output with a record instead.

Measured on the MI355X: worst err / own channel maximum 7.8e-6 under the four 32-row forms (64/2/32, 64/3/32, 128/2/32, 128/3/32) and
6.6e-6 under the two 16-row forms (64/3/16, 128/3/16); pixel-spread case: at most 0.15 of the derived bound under every form, err /
pixel maximum 1.2e-7 at the step 2^0, 8.1e-5 at 2^-12, 2.7e-4 at 2^-13, 1.6e-2 at 2^-16.  The file's 160 tests run in 5.3 s.
"""
import functools
import time

import numpy as np
import pytest
import torch

import conv_ref as ref
import fx3_col_cases as K
from test_hip_f16x3 import planes_match
from test_hip_f16x3_forms import WORST, nchw, per_channel
from test_hip_fp32_plans import SENT, SLOPE, Buf, dev, rnd, spread
from wg3_cases import ints

pytestmark = pytest.mark.gpu

FORMS = list(K.COL_FORMS)
STASH = {}                 # (case, what) -> bytes of the first form's exact-integer result
BETA_MIN = 1e-6


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    t0 = time.time()
    yield functional
    for form in FORMS:
        if "col " + form in WORST:
            print(f"[f16x3 col forms] worst err / own channel maximum, {form}: {WORST['col ' + form]:.2e}")
    print(f"[f16x3 col forms] run time {time.time() - t0:.1f} s")


@pytest.fixture(scope="module")
def lib(F):
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


def ran(lib):
    return tuple(int(lib.stem_tuning_get(k)) for k in (b"fx3_col_ran_tile", b"fx3_col_ran_depth", b"fx3_col_ran_mfma"))


def bias_of(pre, b):
    return pre if b is None else pre + np.asarray(b, np.float64)[None, :, None, None]


@functools.lru_cache(maxsize=None)
def problem(name, kind):
    """operands on the device (split / packed by the library's own kernels) and the float64 convolution before bias"""
    from spatiotemporalentropymodel_amd import functional as F
    B, C, H, W, N, R, S, st, pad = K.COL_SHAPES[name]
    if kind == "ints":
        x, w, b = ints((B, C, H, W), 21, 8.0), ints((N, C, R, S), 22, -8.0), ints((N,), 23, 8.0)
    elif kind == "resid":
        x, w = K.col_resid_operands(name)
        b = None
    else:
        sn = spread(N)
        x = rnd((B, C, H, W), 1)
        w = (rnd((N, C, R, S), 2) / np.sqrt(C * R * S)).astype(np.float32) * sn[:, None, None, None]
        b = rnd((N,), 3) * sn
    return dict(name=name, dims=(B, H, W, C, N, R, S, st, pad), x=x, w=w, b=b, xp=F.F16Planes.split(dev(x)), wp=F.pack_weight_f16x2(dev(w)),
                bias=None if b is None else dev(b), pre=ref.conv2d_fwd(x, w, None, st, pad))


@functools.lru_cache(maxsize=None)
def gdn_params(N, seed=0):
    """stored beta / gamma with entries below their reparametrisation bounds (gamma: 2^-18; beta: sqrt(1e-6 + 2^-36))"""
    from spatiotemporalentropymodel_amd import functional as F
    beta = rnd((N,), 14 + seed, 0.5, 1.5)
    gamma = (rnd((N, N), 15 + seed, 0.0, 0.1) + 0.1 * np.eye(N, dtype=np.float32)).astype(np.float32)
    gamma[0, :4] = [0.0, 1e-7, -0.5, 3.0e-6]
    gamma[N - 1, N - 1] = 1e-6
    beta[1] = 1e-4
    return beta, gamma, dev(beta), F.pack_gdn_gamma_f16x2(dev(gamma))


def launch(F, lib, q, entry, bias, yb, yp, yq, act=0, slope=0.0, beta=None, gp=None):
    B, H, W, C, N, R, S, st, pad = q["dims"]
    xp = q["xp"]
    y, ldy = (0, 0) if yb is None else (yb.ptr, yb.ld)
    ypp = None if yp is None else yp.data.data_ptr()
    b = 0 if bias is None else bias.data_ptr()
    if entry == "act":
        return lib.stem_conv2d_f16x3_fwd_act(xp.data_ptr(), xp.q_ptr(), q["wp"].data_ptr(), b, act, slope, y, ldy, ypp, yq, B, H, W, C, N, R, S, st, pad,
                                             F._stream())
    return lib.stem_conv2d_f16x3_fwd(xp.data_ptr(), xp.q_ptr(), q["wp"].data_ptr(), b, 0 if beta is None else beta.data_ptr(),
                                     0 if gp is None else gp.data_ptr(), BETA_MIN, y, ldy, ypp, yq, B, H, W, C, N, R, S, st, pad, F._stream())


def run_forced(F, lib, q, form, entry, want, what, bias=None, out="fp32", gate=True, exact=False, view=(12, 8), **epi):
    """one forced instantiation, launched twice; out: "fp32" (no record), "planes" (fp32 + planes + record) or "record" (fp32 +
    record, no planes) -> (fp32 output [B,N,OH,OW], planes or None, record or None) of the first launch"""
    B, H, W, C, N, R, S, st, pad = q["dims"]
    sel, inst = K.COL_FORMS[form]
    OH, OW = K.out_hw(H, W, R, S, st, pad)
    slots = K.cdiv(B * OH * OW, inst[0])
    what = f"{what} {form}"
    outs = []
    with F.tuning(**sel):
        for _ in range(2):
            yb = Buf((B, N, OH, OW), N + view[0], view[1])
            yp = rec = None
            if out == "planes":
                yp = F.F16Planes.empty(B, N, OH, OW, torch.device("cuda"))
                yp.data.zero_()
            elif out == "record":
                rec = torch.full((16 + slots + 8,), SENT, device="cuda", dtype=torch.float32)
            rc = launch(F, lib, q, entry, bias, yb, yp, yp.q_ptr() if yp is not None else rec.data_ptr() if rec is not None else None, **epi)
            assert rc == 0, (what, lib.stem_last_error())
            assert ran(lib) == K.col_instantiation(sel["fx3_tile"], sel["fx3_depth"], sel["fx3_mfma"]) == inst, (what, ran(lib))
            outs.append((yb, yp, rec))
        torch.cuda.synchronize()
    yb, yp, rec = outs[0]
    got = yb.host()
    assert torch.equal(yb.buf.view(torch.int32), outs[1][0].buf.view(torch.int32)), what + ": the second launch differs"
    if yp is not None:
        assert torch.equal(yp.data, outs[1][1].data), what + ": planes / scale record of the second launch differ"
    if rec is not None:
        assert torch.equal(rec.view(torch.int32), outs[1][2].view(torch.int32)), what + ": scale record of the second launch differs"
    for o in outs:
        assert o[0].others_untouched(), what + ": wrote outside its channel slice"
    assert not np.isnan(got).any(), what + ": NaN in the output"
    if exact:
        assert np.array_equal(got.astype(np.float64), want), f"{what}: {int((got != want).sum())} elements differ from float64, worst {np.abs(got - want).max():.3e}"
        first = STASH.setdefault((q["name"], what.rsplit(" ", 1)[0]), got.tobytes())
        assert first == got.tobytes(), what + ": the forms do not agree to the bit"
    elif gate:
        per_channel(got, want, what, "col " + form)
    if yp is not None:
        if gate and not exact:
            per_channel(nchw(yp.merge()), want, what + " planes", abs_floor=2.0 ** -24 * yp.record()[0])
        assert planes_match(yp, yb.nchw()), what + ": planes output against the fp32 output of the same launch"
    if rec is not None:
        r = rec.cpu()
        ns = int(r[:1].view(torch.int32)[0])
        assert ns == slots and float(r[1]) == 1.0 and not r[2:16].any(), (what, ns, slots, r[:16])
        assert float(r[16:16 + ns].max()) == float(np.abs(got).max()) and bool((r[16 + ns:] == SENT).all()), what + ": record's maximum"
    return got, yp, rec


def rich(N):
    return "planes" if N % 32 == 0 else "record"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(K.COL_SHAPES))
def test_forced_instantiation_bias_entry(F, lib, name, form):
    """stem_conv2d_f16x3_fwd without GDN: integer inputs (exact, all forms to the bit), systematic residuals, random inputs with
    spread channels; bias / no bias; fp32 only, planes (or a record without planes where N % 32 != 0)"""
    N = K.COL_SHAPES[name][4]
    p = problem(name, "ints")
    run_forced(F, lib, p, form, "fwd", bias_of(p["pre"], p["b"]), f"{name} integers", bias=p["bias"], exact=True, out=rich(N))
    if name in K.COL_RESID:
        p = problem(name, "resid")
        run_forced(F, lib, p, form, "fwd", p["pre"], f"{name} residuals", out=rich(N))
    p = problem(name, "rand")
    run_forced(F, lib, p, form, "fwd", bias_of(p["pre"], p["b"]), f"{name} bias", bias=p["bias"], out=rich(N))
    run_forced(F, lib, p, form, "fwd", p["pre"], f"{name} no bias")
    if N % 32 == 0:
        run_forced(F, lib, p, form, "fwd", bias_of(p["pre"], p["b"]), f"{name} record only", bias=p["bias"], out="record", view=(0, 0))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(K.COL_SHAPES))
def test_forced_instantiation_activation_entry(F, lib, name, form):
    """stem_conv2d_f16x3_fwd_act: integers with the exact slope 0.5 on every shape; slope 0.01 and act = 0 on the COL_ACT shapes"""
    N = K.COL_SHAPES[name][4]
    p = problem(name, "ints")
    run_forced(F, lib, p, form, "act", ref.lrelu(bias_of(p["pre"], p["b"]), 0.5), f"{name} integers lrelu 0.5", bias=p["bias"], exact=True, out=rich(N),
               act=1, slope=0.5)
    if name not in K.COL_ACT:
        return
    p = problem(name, "rand")
    run_forced(F, lib, p, form, "act", ref.lrelu(bias_of(p["pre"], p["b"]), SLOPE), f"{name} lrelu", bias=p["bias"], out=rich(N), act=1, slope=SLOPE)
    run_forced(F, lib, p, form, "act", ref.lrelu(p["pre"], SLOPE), f"{name} lrelu no bias", act=1, slope=SLOPE)
    run_forced(F, lib, p, form, "act", bias_of(p["pre"], p["b"]), f"{name} act 0", bias=p["bias"], act=0, slope=SLOPE)
    if name in K.COL_RESID:
        p = problem(name, "resid")
        run_forced(F, lib, p, form, "act", p["pre"], f"{name} residuals lrelu", out=rich(N), act=1, slope=SLOPE)


@functools.lru_cache(maxsize=None)
def dgrad_problem(kind):
    """the input gradient of Conv2d(96 -> 64, 3x3, padding 1) on 9 x 11: the kernel contracts the layer's 64 OUTPUT channels and its
    output channels are the layer's 96 inputs (pack_weight_f16x2(flip=True): rows = input channels, taps mirrored)"""
    from spatiotemporalentropymodel_amd import functional as F
    B, Cin, H, W, Kout, R = 2, 96, 9, 11, 64, 3
    if kind == "ints":
        dy, w = ints((B, Kout, H, W), 31, -8.0), ints((Kout, Cin, R, R), 32, 8.0)
    elif kind == "resid":
        from wg3_cases import resid
        dy, w = resid((B, Kout, H, W), 33, 5), resid((Kout, Cin, R, R), 34, -14)
    else:
        dy = rnd((B, Kout, H, W), 35)
        w = (rnd((Kout, Cin, R, R), 36) / np.sqrt(Kout * R * R)).astype(np.float32) * spread(Cin)[None, :, None, None]
    return dict(name="dgrad_" + kind, dims=(B, H, W, Kout, Cin, R, R, 1, R // 2), xp=F.F16Planes.split(dev(dy)), wp=F.pack_weight_f16x2(dev(w), flip=True),
                pre=ref.conv2d_dx(dy, w, (B, Cin, H, W), 1, R // 2))


@pytest.mark.parametrize("form", FORMS)
def test_input_gradient_role(F, lib, form):
    """the flipped pack through stem_conv2d_f16x3_fwd_act (act = 0, no bias: layers.py's input gradient of a stride-1 layer)
    against conv_ref.conv2d_dx; and with the leaky-ReLU epilogue on top"""
    p = dgrad_problem("ints")
    run_forced(F, lib, p, form, "act", p["pre"], "input gradient integers", exact=True, out="planes")
    p = dgrad_problem("resid")
    run_forced(F, lib, p, form, "act", p["pre"], "input gradient residuals")
    p = dgrad_problem("rand")
    run_forced(F, lib, p, form, "act", p["pre"], "input gradient", out="planes")
    run_forced(F, lib, p, form, "act", ref.lrelu(p["pre"], SLOPE), "input gradient lrelu", act=1, slope=SLOPE)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", K.COL_GDN)
def test_forced_instantiation_fused_gdn(F, lib, name, form):
    """stem_conv2d_f16x3_fwd with beta / packed gamma: y = v / sqrt(beta' + gamma' v^2) against conv_ref.gdn_fwd, gamma entries and
    one beta below their reparametrisation bounds; fp32 only, planes (record only where N % 32 != 0), bias / no bias"""
    N = K.COL_SHAPES[name][4]
    beta, gamma, bdev, gp = gdn_params(N)
    p = problem(name, "rand")
    want = ref.gdn_fwd(bias_of(p["pre"], p["b"]), beta, gamma, beta_min=BETA_MIN)
    run_forced(F, lib, p, form, "fwd", want, f"{name} gdn", bias=p["bias"], out=rich(N), beta=bdev, gp=gp)
    run_forced(F, lib, p, form, "fwd", ref.gdn_fwd(p["pre"], beta, gamma, beta_min=BETA_MIN), f"{name} gdn no bias", beta=bdev, gp=gp)
    if N % 32 == 0:
        run_forced(F, lib, p, form, "fwd", want, f"{name} gdn record only", bias=p["bias"], out="record", view=(0, 0), beta=bdev, gp=gp)
    p = problem(name, "ints")                       # not exact (the division), but the forms' first contraction is: gate only
    run_forced(F, lib, p, form, "fwd", ref.gdn_fwd(bias_of(p["pre"], p["b"]), beta, gamma, beta_min=BETA_MIN), f"{name} gdn integers", bias=p["bias"],
               beta=bdev, gp=gp)


@pytest.mark.parametrize("name", ["n3_1x3_pad0", "n1_xcd_remap"])
def test_planes_output_needs_32_channel_slabs(F, lib, name):
    p = problem(name, "rand")
    B, H, W, C, N, R, S, st, pad = p["dims"]
    OH, OW = K.out_hw(H, W, R, S, st, pad)
    for entry in ("fwd", "act"):
        yb, yq = Buf((B, N, OH, OW)), torch.zeros(64 + K.cdiv(B * OH * OW, 64), device="cuda")
        assert launch(F, lib, p, entry, p["bias"], yb, F.F16Planes.empty(B, 128, OH, OW, torch.device("cuda")), yq.data_ptr()) != 0
        assert b"planes output needs N % 32 == 0" in lib.stem_last_error() and bool((yb.buf == SENT).all().item()) and not bool(yq.any().item())


@pytest.mark.parametrize("tile", [64, 128])
def test_mfma16_with_the_two_stage_loop_runs_the_32_row_shape(F, lib, tile):
    """`m16 = depth == 3 && ...`: conv_f16x3_kernel<BM, 2, 16> does not exist; the read-back says what ran, and the result is the
    <BM, 2, 32> launch's to the bit"""
    p = problem("n3_1x3_pad0", "rand")
    B, H, W, C, N, R, S, st, pad = p["dims"]
    OH, OW = K.out_hw(H, W, R, S, st, pad)
    res = []
    for mfma in (16, 32):
        with F.tuning(fx3_tile=tile, fx3_depth=2, fx3_mfma=mfma):
            yb = Buf((B, N, OH, OW))
            assert launch(F, lib, p, "fwd", p["bias"], yb, None, None) == 0, lib.stem_last_error()
            assert ran(lib) == K.col_instantiation(tile, 2, mfma) == (tile, 2, 32)
            res.append(yb.host())
    assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32))
    for mfma in (16, 32):
        with F.tuning(fx3_tile=tile, fx3_depth=3, fx3_mfma=mfma):
            assert launch(F, lib, p, "fwd", p["bias"], Buf((B, N, OH, OW)), None, None) == 0
            assert ran(lib) == (tile, 3, mfma)


@functools.lru_cache(maxsize=None)
def zero_image_problem():
    from spatiotemporalentropymodel_amd import functional as F
    B, C, H, W, N = 2, 32, 15, 20, 96
    x = rnd((B, C, H, W), 41)
    x[1] = 0.0
    w = (rnd((N, C, 1, 1), 42) / np.sqrt(C)).astype(np.float32) * spread(N)[:, None, None, None]
    return dict(name="zero_image", dims=(B, H, W, C, N, 1, 1, 1, 0), xp=F.F16Planes.split(dev(x)), wp=F.pack_weight_f16x2(dev(w)),
                pre=ref.conv2d_fwd(x, w, None, 1, 0))


@pytest.mark.parametrize("form", FORMS)
def test_gdn_of_a_zero_image(F, lib, form):
    """second image all zeros, no bias: tiles whose convolution output is exactly zero (vm = 0) -> exact zeros, finite records"""
    p = zero_image_problem()
    B, H, W, C, N = p["dims"][:5]
    bm = K.COL_FORMS[form][1][0]
    assert any(t * bm >= H * W and (t + 1) * bm <= B * H * W for t in range(K.cdiv(B * H * W, bm))), "no tile lies entirely in the zero image"
    assert (H * W) % bm                                             # ... and one straddles the two images
    beta, gamma, bdev, gp = gdn_params(N)
    want = ref.gdn_fwd(p["pre"], beta, gamma, beta_min=BETA_MIN)
    got, yp, _ = run_forced(F, lib, p, form, "fwd", want, "zero image gdn", out="planes", beta=bdev, gp=gp)
    assert not got[1].any(), "the zero image's outputs are not exact zeros"
    inv, amax = yp.record()
    assert np.isfinite(inv) and inv > 0 and amax == float(np.abs(got).max()) and not bool(nchw(yp.merge())[1].any())
    got, _, rec = run_forced(F, lib, p, form, "fwd", want, "zero image gdn record only", out="record", beta=bdev, gp=gp)
    assert not got[1].any() and bool(torch.isfinite(rec[:16 + K.cdiv(B * H * W, bm)]).all())
    got, _, _ = run_forced(F, lib, p, form, "act", ref.lrelu(p["pre"], SLOPE), "zero image lrelu", out="planes", act=1, slope=SLOPE)
    assert not got[1].any()


@functools.lru_cache(maxsize=None)
def pixel_spread_arrays():
    """1x1, C = 32 -> N = 96, 128 pixels = two 64-pixel tiles with the same pattern: pixel p holds the base pattern times
    2^(30 - k), k = (p % 64) % 17; no bias, so the convolution output of a pixel is its base output times 2^(30 - k) and gamma' v^2
    (>= 2^28 times a few) dominates beta' (about 1) at every step"""
    B, C, H, W, N = 1, 32, 8, 16, 96
    k = K.pixel_steps(H * W).reshape(1, 1, H, W)
    base = rnd((B, C, H // 4, W // 2), 51, 0.25, 1.0) * np.where(rnd((B, C, H // 4, W // 2), 52) > 0, 1.0, -1.0).astype(np.float32)
    x = (np.tile(base, (1, 1, 4, 2)) * np.float32(2.0) ** (30 - k)).astype(np.float32)             # [2 x 16] base pixels, 64 + 64 pixels
    w = (rnd((N, C, 1, 1), 53) / np.sqrt(C)).astype(np.float32)
    return dict(name="pixel_spread", dims=(B, H, W, C, N, 1, 1, 1, 0), x=x, w=w, k=k, pre=ref.conv2d_fwd(x, w, None, 1, 0),
                l1=ref.conv2d_fwd(np.abs(x), np.abs(w), None, 1, 0))


@functools.lru_cache(maxsize=None)
def pixel_spread_problem():
    from spatiotemporalentropymodel_amd import functional as F
    p = dict(pixel_spread_arrays())
    p.update(xp=F.F16Planes.split(dev(p["x"])), wp=F.pack_weight_f16x2(dev(p["w"])))
    return p


def pixel_spread_bound(p, beta, gamma, tile=64):
    """(ref, tol, E) per element: the derivation of the module docstring, from the float64 reference alone"""
    v, l1 = p["pre"], p["l1"]
    B, N, H, W = v.shape
    bp, gpm = ref.gdn_params(beta, gamma, BETA_MIN)
    norm = ref.gdn_norm(v, beta, gamma, BETA_MIN)
    want = v / np.sqrt(norm)
    vm = np.abs(v).transpose(0, 2, 3, 1).reshape(-1, tile, N).max(axis=(1, 2))               # the tile's maximum
    assert len(set(vm)) == 1, "the tiles do not share one maximum"
    lg = np.log2(vm[0])
    assert 0.02 < lg - np.floor(lg) < 0.98, "the tile's maximum sits on a binade edge: the fp32 maximum could round to the other side"
    ev = 6 - int(np.floor(lg))                                                               # vm 2^ev in [2^6, 2^7): q_exp(vm) - 8
    d = K.square_split_error((v * 2.0 ** ev) ** 2)
    E = 0.5 * np.einsum("ij,bjhw->bihw", gpm, d) / (norm * 2.0 ** (2 * ev))
    tol = 2.0 ** -20 * l1 / np.sqrt(norm) + np.abs(want) * (2.0 * E + 2.0 ** -18)
    assert (np.einsum("ij,bjhw->bihw", gpm, v ** 2) > 1e3 * bp[None, :, None, None]).all(), "beta' is not negligible at every step"
    return want, tol, E


@pytest.mark.parametrize("form", FORMS)
def test_gdn_of_pixels_far_below_their_tiles_maximum(F, lib, form):
    """the per-element bound derived from the tile-maximum scale of the squares (module docstring); the kernel is held to it"""
    p = pixel_spread_problem()
    N = p["dims"][4]
    beta, gamma, bdev, gp = gdn_params(N)
    want, tol, E = pixel_spread_bound(p, beta, gamma)
    k = np.broadcast_to(p["k"], want.shape)
    # the derivation's own consequence: at the top steps the squares' share is 2^-23; a pixel's values lie below its step (the tile's
    # maximum is one element's), so here it passes 1e-4 between the steps 2^-10 and 2^-12 and is 0.06 .. 0.18 at 2^-16
    assert E[k == 0].max() < 2.0 ** -22 and E[k <= 10].max() < 1e-4 < E[k == 16].min()
    got, yp, _ = run_forced(F, lib, p, form, "fwd", want, "pixel spread gdn", out="planes", gate=False, beta=bdev, gp=gp)
    err = np.abs(got.astype(np.float64) - want)
    pix_max = np.abs(want).max(axis=1, keepdims=True)
    for step in range(K.PIX_STEPS):
        m = k == step
        print(f"[pixel spread] {form} step 2^-{step}: worst err / pixel maximum {(err / pix_max)[m].max():.2e}, worst err / bound {(err / tol)[m].max():.2e}, "
              f"bound / |ref| up to {(tol / np.abs(want))[m].max():.2e}")
    worst = np.unravel_index(np.argmax(err / tol), err.shape)
    assert (err <= tol).all(), f"pixel spread {form}: element {worst} (step 2^-{int(k[worst])}): err {err[worst]:.3e} > derived bound {tol[worst]:.3e}"
    # the convolution alone (no squares involved) keeps every pixel: 2^-20 of its l1 sum
    conv, _, _ = run_forced(F, lib, p, form, "fwd", p["pre"], "pixel spread conv", gate=False)
    assert (np.abs(conv.astype(np.float64) - p["pre"]) <= 2.0 ** -20 * p["l1"]).all(), "the convolution itself loses the small pixels"
