"""GPU: the first-layer kernel c4gdn_f16x3_kernel<NB> (csrc/c4gdn_f16x3.hip: 3-channel image -> N = 64 | 128 | 192 channels + GDN in
one launch) behind stem_conv2d_c4_gdn_f16x3, through the C ABI.  Nothing is forced and nothing read back: the instantiation follows
N (NB = N / 32), which every case states.  Shapes: tests/fx3_col_cases.py C4_SHAPES, pinned on the CPU by
tests/test_fx3_col_plan_abi.py -- N in {64, 128, 192}, windows 1x1, 3x3, 5x5 and 3x5, strides 1 .. 3, pad 0 and R / 2, one output
pixel, a partial last workgroup (128 pixels each), rows longer than a workgroup, bias present / absent, fp32, planes, a record
without planes, output into a channel slice (ldy = N + 12).

Gate: every output channel within 1e-4 of ITS OWN maximum against float64 (conv_ref.gdn_fwd of conv_ref.conv2d_fwd), no floor;
the weights and the bias carry output channel k at the scale 2^(-20 k / (N - 1)); gamma entries and one beta lie below their
reparametrisation bounds.

Exact relations asserted on top:
  * systematic residuals (wg3_cases.resid) on image and weights, in the regime beta' >> gamma' v^2 where the GDN passes a relative
    change of v on: each cross product of the CONVOLUTION carries more than the gate of every output (shown on the CPU).  The
    second contraction's cross products are not reachable this way (its operands are computed, not given);
  * the same launch twice is bit-identical, fp32, planes and scale records byte for byte; sentinels outside the channel slice
    are untouched; no NaN; planes against the fp32 copy of the same launch (test_hip_f16x3.planes_match);
  * a batch whose second image is zero, without bias: exact zeros there (whole workgroups), finite record;
  * pixels that step down to 2^-16 of the image's maximum: held PER ELEMENT to the bound this kernel's own scaling gives.  The
    squares are scaled by the BOUND vb = 3 R S |x|max |w|max + |bias|max of the convolution output (vb^2 2^se in [2^14, 2^15); one
    scale for the launch, not the tile's measured maximum as in the 192-column kernel) and stored as two fp16 numbers, which miss
    up to d(t^2) = max(2^-22 t^2, 2^-25), t = v 2^(se / 2).  With E_i = 1/2 sum_j gamma'_ij d(t_j^2) / (norm_i 2^se):
        |y_i - ref_i| <= 2^-20 l1_i / sqrt(norm_i) + |ref_i| (2 E_i + 2^-18)
    (the terms as in tests/test_hip_f16x3_col_forms.py).  Consequence: a value at rho of the bound vb has its norm
    off by up to 2^-25 / (rho^2 2^14 .. 2^15), its output by half of that -- 1e-4 per element is no longer met below rho = 2^-13.4
    .. 2^-13.9 of the bound, and the bound lies a factor 3 R S |x|max |w|max / max|v| above the values that occur.

Exclusions -- refused by the library with an error (asserted): N outside {64, 128, 192}, windows of more than 25 taps.

Measured on the MI355X: worst err / own channel maximum 9.2e-6 (N = 64), 2.0e-6 (N = 128), 1.7e-6 (N = 192); pixel-spread case: at most
0.15 of the derived bound, err / pixel maximum 1.8e-7 at the step 2^0, 2.9e-5 at 2^-12, 2.1e-2 at 2^-16.  The file's 9 tests run in
3.6 s.
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
from test_hip_fp32_plans import SENT, Buf, dev, rnd, spread

pytestmark = pytest.mark.gpu

BETA_MIN = 1e-6


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    t0 = time.time()
    yield functional
    for N in (64, 128, 192):
        if f"c4gdn {N}" in WORST:
            print(f"[c4gdn forms] worst err / own channel maximum, N = {N}: {WORST[f'c4gdn {N}']:.2e}")
    print(f"[c4gdn forms] run time {time.time() - t0:.1f} s")


@pytest.fixture(scope="module")
def lib(F):
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


def bias_of(pre, b):
    return pre if b is None else pre + np.asarray(b, np.float64)[None, :, None, None]


def gdn_arrays(N):
    beta = rnd((N,), 14, 0.5, 1.5)
    gamma = (rnd((N, N), 15, 0.0, 0.1) + 0.1 * np.eye(N, dtype=np.float32)).astype(np.float32)
    gamma[0, :4] = [0.0, 1e-7, -0.5, 3.0e-6]                     # below the reparametrisation bound 2^-18
    gamma[N - 1, N - 1] = 1e-6
    beta[1] = 1e-4                                               # below sqrt(1e-6 + 2^-36)
    return beta, gamma


def on_device(p):
    """the image as NHWC4 with its scale record, the A-operand stream (C4-packed weights + reparametrised gamma), bias, beta"""
    from spatiotemporalentropymodel_amd import functional as F
    N, R, S = p["dims"][3:6]
    x4 = F.nchw3_to_nhwc4(dev(p["x"]))
    ast = F.c4gdn_stream(F.pack_weight(dev(p["w"]), F.PACK_CONV_FWD_C4), dev(p["gamma"]), N, R, S)
    p.update(x4=x4, ast=ast, bias=None if p["b"] is None else dev(p["b"]), bdev=dev(p["beta"]))
    return p


@functools.lru_cache(maxsize=None)
def problem(name, kind):
    B, H, W, N, R, S, st, pad = K.C4_SHAPES[name]
    beta, gamma = gdn_arrays(N)
    if kind == "resid":
        x, w = K.c4_resid_operands(name)
        b = None
    else:
        sn = spread(N)
        x = rnd((B, 3, H, W), 81, 0.0, 1.0)
        w = (rnd((N, 3, R, S), 82) / np.sqrt(3 * R * S)).astype(np.float32) * sn[:, None, None, None]
        b = (rnd((N,), 83, -0.1, 0.1) * sn).astype(np.float32)
    return on_device(dict(name=name, dims=(B, H, W, N, R, S, st, pad), x=x, w=w, b=b, beta=beta, gamma=gamma, pre=ref.conv2d_fwd(x, w, None, st, pad)))


def launch(F, lib, p, bias, yb, yp, yq):
    B, H, W, N, R, S, st, pad = p["dims"]
    return lib.stem_conv2d_c4_gdn_f16x3(p["x4"].data_ptr(), F._nhwc4_record(p["x4"]).data_ptr(), p["ast"].data_ptr(), 0 if bias is None else bias.data_ptr(),
                                        p["bdev"].data_ptr(), BETA_MIN, 0 if yb is None else yb.ptr, 0 if yb is None else yb.ld,
                                        None if yp is None else yp.data.data_ptr(), yq, B, H, W, N, R, S, st, pad, F._stream())


def run(F, lib, p, want, what, bias=None, out="fp32", gate=True, view=(12, 8)):
    """launched twice; out: "fp32", "planes" (fp32 + planes + record) or "record" (fp32 + record) -> (fp32 [B,N,OH,OW], planes, record)"""
    B, H, W, N, R, S, st, pad = p["dims"]
    OH, OW = K.out_hw(H, W, R, S, st, pad)
    slots = K.cdiv(B * OH * OW, K.C4_WG)
    outs = []
    for _ in range(2):
        yb = Buf((B, N, OH, OW), N + view[0], view[1])
        yp = rec = None
        if out == "planes":
            yp = F.F16Planes.empty(B, N, OH, OW, torch.device("cuda"))
            yp.data.zero_()
        elif out == "record":
            rec = torch.full((16 + slots + 8,), SENT, device="cuda", dtype=torch.float32)
        rc = launch(F, lib, p, bias, yb, yp, yp.q_ptr() if yp is not None else rec.data_ptr() if rec is not None else None)
        assert rc == 0, (what, lib.stem_last_error())
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
    if gate:
        per_channel(got, want, what, f"c4gdn {N}")
    if yp is not None:
        if gate:
            per_channel(nchw(yp.merge()), want, what + " planes", abs_floor=2.0 ** -24 * yp.record()[0])
        assert planes_match(yp, yb.nchw()), what + ": planes output against the fp32 output of the same launch"
    if rec is not None:
        r = rec.cpu()
        n = int(r[:1].view(torch.int32)[0])
        assert n == slots and float(r[1]) == 1.0 and not r[2:16].any(), (what, n, slots, r[:16])
        assert float(r[16:16 + n].max()) == float(np.abs(got).max()) and bool((r[16 + n:] == SENT).all()), what + ": record's maximum"
    return got, yp, rec


def gdn_of(p, v):
    return ref.gdn_fwd(v, p["beta"], p["gamma"], beta_min=BETA_MIN)


@pytest.mark.parametrize("name", list(K.C4_SHAPES))
def test_first_layer_shapes(F, lib, name):
    """bias / no bias; fp32 only into a channel slice, planes, record without planes (dense rows); residual inputs"""
    p = problem(name, "rand")
    want = gdn_of(p, bias_of(p["pre"], p["b"]))
    run(F, lib, p, want, f"{name} fp32", bias=p["bias"])
    run(F, lib, p, want, f"{name} planes", bias=p["bias"], out="planes")
    run(F, lib, p, want, f"{name} record only", bias=p["bias"], out="record", view=(0, 0))
    run(F, lib, p, gdn_of(p, p["pre"]), f"{name} no bias", out="planes")
    p = problem(name, "resid")
    run(F, lib, p, gdn_of(p, p["pre"]), f"{name} residuals")


def test_refusals(F, lib):
    p = problem("1x1_s3_n64", "rand")
    B, H, W, N, R, S, st, pad = p["dims"]
    for n, r, s in ((96, 1, 1), (32, 1, 1), (256, 1, 1), (64, 5, 7), (64, 6, 5)):
        assert not lib.stem_c4gdn_supported(n, r, s) and lib.stem_c4gdn_stream_bytes(n, r, s) == 0
        yb = Buf((B, 64, 4, 5))
        q = dict(p, dims=(B, H, W, n, r, s, st, pad))
        assert launch(F, lib, q, None, yb, None, None) != 0 and b"N must be 64, 128 or 192 and R*S <= 25" in lib.stem_last_error()
        assert bool((yb.buf == SENT).all().item())
        assert lib.stem_c4gdn_pack(p["ast"].data_ptr(), p["ast"].data_ptr(), p["ast"].data_ptr(), n, r, s, F._stream()) != 0
        assert b"N must be 64, 128 or 192 and R*S <= 25" in lib.stem_last_error()
    for n in (64, 128, 192):
        assert lib.stem_c4gdn_supported(n, 5, 5) and lib.stem_c4gdn_supported(n, 3, 5) and lib.stem_c4gdn_supported(n, 1, 1)
    yb = Buf((B, N, 4, 5), N + 6, 2)                                  # rows that are not 16-byte aligned
    assert launch(F, lib, p, None, yb, None, None) != 0 and b"16-byte aligned" in lib.stem_last_error()


@functools.lru_cache(maxsize=None)
def zero_image_problem():
    B, H, W, N, R = 2, 15, 20, 128, 3
    beta, gamma = gdn_arrays(N)
    x = rnd((B, 3, H, W), 84, 0.0, 1.0)
    x[1] = 0.0
    w = (rnd((N, 3, R, R), 85) / np.sqrt(27)).astype(np.float32) * spread(N)[:, None, None, None]
    return on_device(dict(name="zero_image", dims=(B, H, W, N, R, R, 1, 1), x=x, w=w, b=None, beta=beta, gamma=gamma, pre=ref.conv2d_fwd(x, w, None, 1, 1)))


def test_gdn_of_a_zero_image(F, lib):
    p = zero_image_problem()
    B, H, W = p["dims"][:3]
    assert any(t * K.C4_WG >= H * W and (t + 1) * K.C4_WG <= B * H * W for t in range(K.cdiv(B * H * W, K.C4_WG))), "no workgroup lies entirely in the zero image"
    want = gdn_of(p, p["pre"])
    got, yp, _ = run(F, lib, p, want, "zero image", out="planes")
    assert not got[1].any(), "the zero image's outputs are not exact zeros"
    inv, amax = yp.record()
    assert np.isfinite(inv) and inv > 0 and amax == float(np.abs(got).max()) and not bool(nchw(yp.merge())[1].any())
    got, _, rec = run(F, lib, p, want, "zero image record only", out="record")
    assert not got[1].any() and bool(torch.isfinite(rec[:16 + K.cdiv(B * H * W, K.C4_WG)]).all())


@functools.lru_cache(maxsize=None)
def pixel_spread_arrays():
    """1x1, 3 -> 64 channels, 128 pixels: pixel p holds a base pattern times 2^(30 - k), k = (p % 64) % 17; no bias, so gamma' v^2
    dominates beta' (about 1) at every step"""
    B, H, W, N = 1, 8, 16, 64
    beta, gamma = gdn_arrays(N)
    k = K.pixel_steps(H * W).reshape(1, 1, H, W)
    base = rnd((B, 3, H, W), 86, 0.25, 1.0) * np.where(rnd((B, 3, H, W), 87) > 0, 1.0, -1.0).astype(np.float32)
    x = (base * np.float32(2.0) ** (30 - k)).astype(np.float32)
    w = (rnd((N, 3, 1, 1), 88) / np.sqrt(3)).astype(np.float32)
    return dict(name="pixel_spread", dims=(B, H, W, N, 1, 1, 1, 0), x=x, w=w, b=None, k=k, beta=beta, gamma=gamma, pre=ref.conv2d_fwd(x, w, None, 1, 0),
                l1=ref.conv2d_fwd(np.abs(x), np.abs(w), None, 1, 0))


def pixel_spread_bound(p):
    """(ref, tol, E) per element: the derivation of the module docstring, from the float64 reference and the kernel's bound vb"""
    v, l1 = p["pre"], p["l1"]
    R, S = p["dims"][4:6]
    bp, gpm = ref.gdn_params(p["beta"], p["gamma"], BETA_MIN)
    norm = ref.gdn_norm(v, p["beta"], p["gamma"], BETA_MIN)
    want = v / np.sqrt(norm)
    vb = np.float32(3 * R * S) * np.float32(np.abs(p["x"]).max()) * np.float32(np.abs(p["w"]).max())          # as the kernel computes it (no bias)
    lg = np.log2(np.float64(vb) ** 2)
    assert 0.02 < lg - np.floor(lg) < 0.98, "the bound's square sits on a binade edge: fp32 could round it to the other side"
    se = 14 - int(np.floor(lg))                                                                              # vb^2 2^se in [2^14, 2^15): q_exp(vb * vb)
    d = K.square_split_error(v ** 2 * 2.0 ** se)
    E = 0.5 * np.einsum("ij,bjhw->bihw", gpm, d) / (norm * 2.0 ** se)
    tol = 2.0 ** -20 * l1 / np.sqrt(norm) + np.abs(want) * (2.0 * E + 2.0 ** -18)
    assert (np.einsum("ij,bjhw->bihw", gpm, v ** 2) > 1e3 * bp[None, :, None, None]).all(), "beta' is not negligible at every step"
    return want, tol, E


def test_gdn_of_pixels_far_below_the_bound(F, lib):
    """the per-element bound derived from the launch-wide scale of the squares (module docstring); the kernel is held to it"""
    p = on_device(dict(pixel_spread_arrays()))
    want, tol, E = pixel_spread_bound(p)
    k = np.broadcast_to(p["k"], want.shape)
    assert E[k == 0].max() < 2.0 ** -21 and E[k <= 10].max() < 1e-4 < E[k == 16].min()
    got, yp, _ = run(F, lib, p, want, "pixel spread", out="planes", gate=False)
    err = np.abs(got.astype(np.float64) - want)
    pix_max = np.abs(want).max(axis=1, keepdims=True)
    for step in range(K.PIX_STEPS):
        m = k == step
        print(f"[pixel spread c4] step 2^-{step}: worst err / pixel maximum {(err / pix_max)[m].max():.2e}, worst err / bound {(err / tol)[m].max():.2e}, "
              f"bound / |ref| up to {(tol / np.abs(want))[m].max():.2e}")
    worst = np.unravel_index(np.argmax(err / tol), err.shape)
    assert (err <= tol).all(), f"pixel spread: element {worst} (step 2^-{int(k[worst])}): err {err[worst]:.3e} > derived bound {tol[worst]:.3e}"
