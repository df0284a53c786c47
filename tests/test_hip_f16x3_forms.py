"""GPU: the general fp16 forward family behind stem_conv2d_f16x3_gen_fwd -- conv_f16x3_gen_kernel with 64- and 128-pixel tiles
and both MFMA shapes (csrc/conv_f16x3.hip), and the image-tile form (csrc/conv_f16x3_img.hip) -- under EVERY form, split and
tile edge, forced through the library's selectors (F.tuning: fx3_gen_img, fx3_gen_tile, fx3_gen_mfma, fx3_split) instead of
left to the planners.  Shapes, forms and the host arithmetic of a launch: tests/fx3_form_cases.py (its split lists are pinned
on the CPU by tests/test_f16x3_plan_abi.py, which also checks that they reach a split that starts mid-slab and one that starts
on a slab's last tap -- the special case of the image-tile prologue, conv_f16x3_img.hip "if (t == T - 1)").

Every case: force a form and a split s; size a workspace of its own with stem_conv2d_f16x3_gen_workspace_bytes queried under
that plan (checked against 65536 + min(s, n) * M * cdiv(N, 128) * 128 * 4, or 0 when min(s, n) == 1; n = (C / 32) * T chunks);
call the C ABI; assert that stem_tuning_get("fx3_ran_form" | "fx3_ran_mfma" | "fx3_ran_split") reports the forced plan with
fx3_ran_split == s_eff = cdiv(n, cdiv(n, min(s, n))); compare with the float64 statements of tests/conv_ref.py.

Gate: every output channel within 1e-4 of ITS OWN maximum against float64, no floor (test_hip_dynrange.per_channel, span 20;
test_hip_fp32_plans).  The channel is the kernel's output channel: the layer's output channel for a forward, its input channel
for the input-gradient role.  Output channel k of the weights and of the bias carries the scale 2^(-20 k / (K - 1)), the bias is
U(-1, 1) times that scale, z holds exact 0.0 and -0.0.  Planes outputs are held to their own layout (test_hip_dynrange: 1e-4 of
the channel's maximum or the grid of the second fp16 number, 2^-24 of the unit in the scale record) and to
test_hip_f16x3.planes_match against the fp32 copy of the same launch.

Exact relations asserted on top (lines of csrc/f16x3_tail.h, the tail both kernels share, unless stated):
  * sentinels outside the output's channel slice are untouched (tail_rows: the stores are `colok && m >= 0` rows of 16 bytes
    at a.y + m * a.ldy + ecol, m = the kernel's output row of the tile row: MOF in conv_f16x3_img.hip, OROW in conv_f16x3.hip);
  * the same forced launch twice into the same workspace is bit-identical, fp32 and planes, scale records included byte for
    byte (tail_slab_sum: "sums the nsplit slabs ... in split order, its own included at its place: one fixed order whoever
    arrives last"; conv_f16x3.hip states the same loop itself; q_header zeroes the reserved words, stem_common.h);
  * after every split launch the first 64 KiB of the workspace are zero (splitk_last_arriver re-arms the counter);
  * POISONED SLABS: before each split launch everything behind the counters is NaN.  A workgroup writes every element of its
    partial tile that lies inside the image (conv_f16x3_img.hip: `if (m >= 0)` stores of all 128 columns, dead wavefronts
    included: their accumulators are zero; conv_f16x3.hip: `if (m < Mtot)`) and the owner reads exactly those
    (conv_f16x3_img.hip: eoff[k] = em[k] >= 0 ? ... : OOR; conv_f16x3.hip: eoff[k] = m < Mtot ? ... : OOR), so a sum that
    includes an element nobody wrote THIS launch is NaN and fails the gate at once; columns >= N and rows outside the image
    are discarded;
  * a forced split with a null workspace runs unsplit ("no workspace: unsplit", conv_f16x3.hip) and equals forced s = 1 to the bit;
  * on the image-tile form conv(2^kx x, 2^kw w) == 2^(kx+kw) conv(x, w) bit for bit (the scale records carry the exponents:
    fac = q_inv(xq) * q_inv(wq) is a power of two), an all-zero input gives exact zeros and the record (1.0, 0.0);
  * fp32 output with a record but no planes (yq set, yp null): the header says inv = 1 (tail_record:
    `if (!planes) yq[1] = 1.f`), one slot per workgroup of the grid's first two dimensions, their maximum is max|y|, and
    stem_f16x2_split_nhwc fed that record as src_q writes the bytes F16Planes.split(y) writes.

Exclusions -- refused by the library with an error (asserted), nothing else is left out:
  * planes output of the N = 132 shape ("planes output needs N % 32 == 0"): fp32 output with a record instead;
  * the input-gradient role of the N = 132 shape: its contraction would have 132 channels ("C % 32 == 0").
The input-gradient role runs on the unmasked shapes only (the engine passes no `taps` there).  Bit equality between the
image-tile and the general forms is not asserted: their chunk walks differ.
"""
import functools

import numpy as np
import pytest
import torch

import conv_ref as ref
from fx3_form_cases import CNT_BYTES, FORMS, GBN, SHAPES, TS, cdiv, chunks, img_eligible_forced, live_taps, s_eff, split_list, workspace_bytes
from test_hip_f16x3 import planes_match
from test_hip_fp32_plans import SENT, SLOPE, Buf, dev, rnd, spread, with_zeros

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_LRELU, EPI_DACT = 0, 1, 2
NAN_BITS = 0x7FC00000
WORST = {}                 # form -> worst err / own channel maximum seen (printed when the module is done)


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield functional
    for form in sorted(WORST):
        print(f"[f16x3 forms] worst err / own channel maximum, {form}: {WORST[form]:.2e}")


@pytest.fixture(scope="module")
def lib(F):
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


def per_channel(a, r, what, form=None, abs_floor=None, rtol=1e-4):
    """every channel within rtol of ITS OWN maximum, no floor; abs_floor (planes outputs only): the grid of the second fp16 number"""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    assert a.shape == r.shape, (what, a.shape, r.shape)
    assert not np.isnan(a).any(), what + ": NaN in the output (a slab element nobody wrote this launch was summed)"
    cmax, err = np.abs(r).max(axis=(0, 2, 3)), np.abs(a - r).max(axis=(0, 2, 3))
    assert cmax.min() > 0, what
    tol = rtol * cmax if abs_floor is None else np.maximum(rtol * cmax, abs_floor)
    ratio = err / cmax
    worst = int(np.argmax(err / tol))
    print(f"[per channel] {what}: worst err / own max {ratio.max():.2e} (channel {int(np.argmax(ratio))}), tensor max {cmax.max():.2e}")
    if form is not None:
        WORST[form] = max(WORST.get(form, 0.0), float(ratio.max()))
    assert (err <= tol).all(), f"{what}: channel {worst}: err {err[worst]:.3e} > {tol[worst]:.3e} (own max {cmax[worst]:.3e})"


def nchw(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


@functools.lru_cache(maxsize=None)
def problem(name):
    """operands on the device (split / packed by the library's own kernels) and the float64 results before bias and activation"""
    from spatiotemporalentropymodel_amd import functional as F
    B, C, H, W, N, R, taps = SHAPES[name]
    T, pad = live_taps(R, taps), R // 2
    sn = spread(N)
    w = (rnd((N, C, R, R), 2) / np.sqrt(C * T)).astype(np.float32) * sn[:, None, None, None]
    mask = None if not taps else ref.mask_a(R, R) if taps == (R // 2) * R + R // 2 else ref.mask_b(R, R)
    assert mask is None or int(mask.sum()) == taps
    wm = w if mask is None else (w * mask).astype(np.float32)
    x, b = rnd((B, C, H, W), 1), rnd((N,), 3) * sn
    wd = dev(w)
    p = dict(name=name, dims=(B, H, W, C, N, R), taps=taps, x=x, b=b, xp=F.F16Planes.split(dev(x)), wp=F.pack_weight_f16x2_gen(wd, taps=taps),
             bias=dev(b), pre=ref.conv2d_fwd(x, wm, None, 1, pad), wm=wm, dgrad=None)
    assert np.array_equal(nchw(wd), wm)                       # a masked pack zeroes the dead taps in place
    if not taps and N % 32 == 0:                              # input-gradient role: the kernel's output channels are the layer's INPUT channels
        sc = spread(C)
        w2 = (rnd((N, C, R, R), 4) / np.sqrt(N * R * R)).astype(np.float32) * sc[None, :, None, None]
        dy, z = rnd((B, N, H, W), 5), with_zeros(rnd((B, C, H, W), 6))
        p["dgrad"] = dict(dims=(B, H, W, N, C, R), taps=0, xp=F.F16Planes.split(dev(dy)), wp=F.pack_weight_f16x2_gen(dev(w2), flip=True), z=z,
                          pre=ref.conv2d_dx(dy, w2, (B, C, H, W), 1, pad))
    return p


def launch(F, lib, q, epi, bias, zb, yb, yp, yq, ws, wsb):
    B, H, W, C, N, R = q["dims"]
    xp = q["xp"]
    return lib.stem_conv2d_f16x3_gen_fwd(xp.data_ptr(), xp.q_ptr(), xp.pix_bytes, q["wp"].data_ptr(), 0 if bias is None else bias.data_ptr(), epi, SLOPE,
                                         0 if zb is None else zb.ptr, 0 if zb is None else zb.ld, 0 if yb is None else yb.ptr, 0 if yb is None else yb.ld,
                                         None if yp is None else yp.data.data_ptr(), yq, B, H, W, C, N, R, R, 1, R // 2, q["taps"],
                                         0 if ws is None else ws.data_ptr(), wsb, F._stream())


def ran(lib):
    return tuple(int(lib.stem_tuning_get(k)) for k in (b"fx3_ran_form", b"fx3_ran_mfma", b"fx3_ran_split"))


def record_slots(form_id, B, H, W, N):
    """workgroups of the grid's first two dimensions: each owns one slot of the output's scale record"""
    ntn = cdiv(N, GBN)
    return B * cdiv(H, TS) * cdiv(W, TS) * ntn if form_id == 3 else cdiv(B * H * W, 64 if form_id == 1 else 128) * ntn


def run_forced(F, lib, q, form, s, epi, want, what, bias=None, z=None, view=(12, 8), planes=False, record=False, null_ws=False, gate=True):
    """one forced plan, launched twice where it splits; -> (fp32 output [B,N,H,W], planes or None, Buf, record or None) of the first launch"""
    B, H, W, C, N, R = q["dims"]
    sel, form_id, mfma = FORMS[form]
    n = chunks(C, R, q["taps"])
    se = 1 if null_ws else s_eff(n, s)
    what = f"{what} {form} split {s} (s_eff {se})"
    if form == "img":
        assert img_eligible_forced(B, H, W, N, R), what
    zb = None if z is None else Buf(z.shape, N + 8, 4, src=z)
    with F.tuning(fx3_split=s, **sel):
        wsb = int(lib.stem_conv2d_f16x3_gen_workspace_bytes(B, H, W, C, N, R, R, 1, R // 2, q["taps"]))
        assert wsb == workspace_bytes(B, H, W, N, n, s), (what, wsb)
        ws = torch.zeros(wsb // 4, device="cuda", dtype=torch.int32) if wsb and not null_ws else None
        outs = []
        for _ in range(2 if se > 1 else 1):
            if ws is not None:
                ws[CNT_BYTES // 4:] = NAN_BITS                   # a slab element that is summed without having been written shows
            yb = Buf((B, N, H, W), N + view[0], view[1])
            yp = rec = None
            if planes:
                yp = F.F16Planes.empty(B, N, H, W, torch.device("cuda"))
                yp.data.zero_()
            elif record:
                rec = torch.full((16 + record_slots(1, B, H, W, N) + 8,), SENT, device="cuda", dtype=torch.float32)
            rc = launch(F, lib, q, epi, bias, zb, yb, yp, yp.q_ptr() if planes else rec.data_ptr() if record else None, ws, 0 if ws is None else wsb)
            assert rc == 0, (what, lib.stem_last_error())
            assert ran(lib) == (form_id, mfma, se), (what, ran(lib))
            outs.append((yb, yp, rec))
        torch.cuda.synchronize()
    yb, yp, rec = outs[0]
    got = yb.host()
    if se > 1:
        assert int(ws[:CNT_BYTES // 4].abs().max().item()) == 0, what + ": arrival counters not left at zero"
        assert torch.equal(yb.buf.view(torch.int32), outs[1][0].buf.view(torch.int32)), what + ": second launch into the same workspace differs"
        if planes:
            assert torch.equal(yp.data, outs[1][1].data), what + ": planes / scale record of the second launch differ"
        if record:
            assert torch.equal(rec.view(torch.int32), outs[1][2].view(torch.int32)), what + ": scale record of the second launch differs"
    for o in outs:
        assert o[0].others_untouched(), what + ": wrote outside its channel slice"
    assert not np.isnan(got).any(), what + ": NaN in the output"
    if gate:
        per_channel(got, want, what, form)
    if planes:
        if gate:
            per_channel(nchw(yp.merge()), want, what + " planes", abs_floor=2.0 ** -24 * yp.record()[0])
        assert planes_match(yp, yb.nchw()), what + ": planes output against the fp32 output of the same launch"
    if record:
        r = rec.cpu()
        ns = int(r[:1].view(torch.int32)[0])
        assert ns == record_slots(form_id, B, H, W, N) and float(r[1]) == 1.0 and not r[2:16].any(), (what, ns, r[:16])
        assert float(r[16:16 + ns].max()) == float(np.abs(got).max()) and bool((r[16 + ns:] == SENT).all()), what + ": record's maximum"
    return got, yp, yb, rec


CASES = [(name, s) for name, (B, C, H, W, N, R, taps) in SHAPES.items() for s in split_list(chunks(C, R, taps))]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-s{c[1]}")
def test_forced_form_and_split(F, lib, case, form):
    """forward (bias + leaky ReLU into a channel slice, planes alongside), the input-gradient role (flipped pack, DACT with z from a
    wider buffer, null bias) on the unmasked shapes, GEN_EPI_BIAS with a record and no planes on the first and third shape"""
    name, s = case
    p = problem(name)
    B, H, W, C, N, R = p["dims"]
    want = ref.lrelu(p["pre"] + p["b"].astype(np.float64)[None, :, None, None], SLOPE)
    if N % 32:
        yb, yq = Buf((B, N, H, W)), torch.zeros(64, device="cuda")
        with F.tuning(**FORMS[form][0]):
            assert launch(F, lib, p, EPI_LRELU, p["bias"], None, yb, F.F16Planes.empty(B, 160, H, W, torch.device("cuda")), yq.data_ptr(), None, 0) != 0
        assert b"planes output needs N % 32 == 0" in lib.stem_last_error() and bool((yb.buf == SENT).all().item())
    run_forced(F, lib, p, form, s, EPI_LRELU, want, f"{name} forward", bias=p["bias"], planes=N % 32 == 0, record=N % 32 != 0)
    d = p["dgrad"]
    if d is not None:
        run_forced(F, lib, d, form, s, EPI_DACT, ref.dact(d["pre"], d["z"], SLOPE), f"{name} input gradient", z=d["z"])
    if name in ("partial_tile_both_ways", "masked_a_column_tail"):
        run_forced(F, lib, p, form, s, EPI_BIAS, p["pre"] + p["b"].astype(np.float64)[None, :, None, None], f"{name} bias only", bias=p["bias"], record=True)


def test_input_gradient_role_needs_32_contraction_channels(F, lib):
    """the N = 132 shape has no input-gradient role on this family: its contraction would have 132 channels"""
    p = problem("1x1_n132")
    B, H, W, C, N, R = p["dims"]
    yb = Buf((B, C, H, W))
    q = dict(dims=(B, H, W, N, C, R), taps=0, xp=p["xp"], wp=p["wp"])
    assert launch(F, lib, q, EPI_BIAS, None, None, yb, None, None, None, 0) != 0 and b"C % 32 == 0" in lib.stem_last_error()
    assert bool((yb.buf == SENT).all().item())


@pytest.mark.parametrize("s", [1, 5])
@pytest.mark.parametrize("form", list(FORMS))
def test_input_read_through_a_channel_view(F, lib, form, s):
    """the input as channels [32, 32 + C) of a planes tensor 32 channels wider: xpix > (C / 32) * 128, the record of the whole tensor"""
    p = problem("partial_tile_both_ways")
    B, H, W, C, N, R = p["dims"]
    big = np.concatenate([3.0 * rnd((B, 32, H, W), 7), p["x"]], axis=1)          # the unread channels set the tensor's scale
    bigp = F.F16Planes.split(dev(big))
    view = bigp.channels(32, 32 + C)
    assert view.pix_bytes == (C // 32 + 1) * 128 and view.data_ptr() == bigp.data_ptr() + 128
    q = dict(p, xp=view)
    run_forced(F, lib, q, form, s, EPI_LRELU, ref.lrelu(p["pre"] + p["b"].astype(np.float64)[None, :, None, None], SLOPE), "channel-view input",
               bias=p["bias"], planes=True)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_forced_split_without_a_workspace_runs_unsplit(F, lib, name, form):
    p = problem(name)
    want = p["pre"] + p["b"].astype(np.float64)[None, :, None, None]
    one = run_forced(F, lib, p, form, 1, EPI_BIAS, want, f"{name} unsplit", bias=p["bias"])[0]
    nul = run_forced(F, lib, p, form, 3, EPI_BIAS, want, f"{name} null workspace", bias=p["bias"], null_ws=True)[0]
    assert np.array_equal(one.view(np.uint32), nul.view(np.uint32)), f"{name} {form}: a forced split without a workspace is not the unsplit launch"


@pytest.mark.parametrize("kx,kw", [(-70, 0), (0, -40), (45, 20), (-30, 50)])
def test_power_of_two_scaling_is_exact_on_the_image_tile_form(F, lib, kx, kw):
    """conv(2^kx x, 2^kw w) == 2^(kx+kw) conv(x, w) bit for bit, fp32 and merged planes, on partial tiles under the 5-way split whose
    third workgroup starts on a slab's last tap; an all-zero input gives exact zeros and the record (1.0, 0.0)"""
    p = problem("partial_tile_both_ways")
    B, H, W, C, N, R = p["dims"]
    f = float(np.float32(2.0 ** kx) * np.float32(2.0 ** kw))

    def run(xs, ws_):
        q = dict(p, xp=F.F16Planes.split(dev(xs)), wp=F.pack_weight_f16x2_gen(dev(ws_)))
        got, yp, yb, _ = run_forced(F, lib, q, "img", 5, EPI_BIAS, None, f"scaling 2^{kx} 2^{kw}", planes=True, view=(0, 0), gate=False)
        return yb.nchw().clone(), yp.merge(), yp.record()

    y0, m0, _ = _scaled(run, p, 1.0, 1.0)
    y1, m1, _ = _scaled(run, p, np.float32(2.0 ** kx), np.float32(2.0 ** kw))
    assert torch.equal(y0 * f, y1), f"fp32 output: scaling the operands by 2^{kx}, 2^{kw} changed more than the exponent"
    assert torch.equal(m0 * f, m1), f"planes output: scaling the operands by 2^{kx}, 2^{kw} changed more than the exponent"
    yz, mz, recz = _scaled(run, p, 0.0, 1.0)
    assert float(yz.abs().max()) == 0.0 and float(mz.abs().max()) == 0.0 and recz == (1.0, 0.0)


def _scaled(run, p, sx, sw):
    return run((p["x"] * np.float32(sx)).astype(np.float32), (p["wm"] * np.float32(sw)).astype(np.float32))


@pytest.mark.parametrize("form", list(FORMS))
def test_record_without_planes_feeds_the_split_kernel(F, lib, form):
    """yq set, yp null: inv = 1, one slot per workgroup, their maximum is max|y| (asserted in run_forced); stem_f16x2_split_nhwc fed
    that record as src_q writes the bytes F16Planes.split(y) writes"""
    p = problem("partial_tile_both_ways")
    want = p["pre"] + p["b"].astype(np.float64)[None, :, None, None]
    _, _, yb, rec = run_forced(F, lib, p, form, 3, EPI_BIAS, want, "record without planes", bias=p["bias"], record=True, view=(0, 0))
    own, fed = F.F16Planes.split(yb.nchw()), F.F16Planes.split(yb.nchw(), src_q=rec.data_ptr())
    torch.cuda.synchronize()
    assert own.q_offset == fed.q_offset and torch.equal(own.data[:own.q_offset], fed.data[:fed.q_offset]), "planes bytes differ"
    assert own.record() == fed.record()


def test_default_planner_chooses_the_documented_form(F, lib):
    """no selector set: the form only (the planners' split numbers are performance choices and are not pinned)"""
    def form_of(B, C, H, W, N, R, **sel):
        x = torch.randn(B, C, H, W, device="cuda")
        w = torch.randn(N, C, R, R, device="cuda") / (C * R * R) ** 0.5
        with F.tuning(**sel):
            F.conv2d_f16x3_gen(F.F16Planes.split(x), F.pack_weight_f16x2_gen(w), None, N, R, R, 1, R // 2)
            torch.cuda.synchronize()
            return int(lib.stem_tuning_get(b"fx3_ran_form"))

    for k in (b"fx3_gen_img", b"fx3_gen_tile", b"fx3_gen_mfma", b"fx3_split"):
        assert lib.stem_tuning_get(k) == 0, k
    assert form_of(4, 192, 16, 16, 256, 5) == 3
    assert form_of(2, 576, 8, 8, 384, 1) in (1, 2)
    assert form_of(16, 64, 64, 64, 256, 3) in (1, 2)             # its 128-pixel form already has two workgroups per CU
    assert form_of(4, 192, 16, 16, 256, 5, fx3_gen_tile=64) == 1 and form_of(4, 192, 16, 16, 256, 5, fx3_gen_tile=128) == 2
