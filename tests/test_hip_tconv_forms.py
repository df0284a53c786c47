"""GPU: the four-phase transposed form conv_f16x3_gen_kernel<GBM, 16, true> (csrc/conv_f16x3.hip) behind stem_tconv2d_f16x3_fwd --
the forward of the stride-2 transposed hyper layers and the input gradient of the stride-2 convolutions -- under BOTH pixel tiles
(F.tuning(fx3_gen_tile = 64 | 128); the planner takes the 128-pixel instantiation only from 4 * cdiv(M, 128) * ntn >= 256 on) and
EVERY per-phase split vector its plans reach, forced through fx3_split (and tconv_cps once) and read back through
stem_tuning_get("tconv_ran_tile" | "tconv_ran_cps" | "tconv_ran_split0" .. "tconv_ran_split3"), which must equal the restatement
fx3_col_cases.tconv_plan: cps = cdiv(maxc, min(s, maxc)), nsplit[p] = cdiv(nch[p], min(cps, nch[p])), and cps = 2^30 with all
phases unsplit where the workspace is null or one byte short of 65536 + 4 * sum(nsplit > 1 ? nsplit * M * ntn * 128 : 0).
Shapes and the host arithmetic: tests/fx3_col_cases.py, pinned on the CPU by tests/test_fx3_col_plan_abi.py: M = B H W in
{70, 54, 84, 144, 72} (below 64, ragged on both tiles), C in {32, 64, 96}, N in {96, 132, 160}, R in {3, 5}, the fine grids
2H x 2W, (2H - 1) x 2W, 2H x (2W - 1), (2H - 1) x (2W - 1); plans with one phase split and three not (1/1/1/2), phases with
different split counts under one blockIdx.z extent, an unsplit phase between split ones (only split phases own slabs), one chunk
per workgroup in every phase, the clamp at s > maxc.

Reference: conv_ref.conv2d_dx on the (odd-sized) fine shape -- the transposed face IS the adjoint of the stride-2 convolution that
maps the fine grid to the coarse one.  Gate: every output channel within 1e-4 of ITS OWN maximum against float64, no floor; random
weights and bias carry output channel k at the scale 2^(-20 k / (N - 1)); z of the DACT epilogue holds exact 0.0 and -0.0.  Planes
outputs: their own layout's gate and test_hip_f16x3.planes_match against the fp32 copy of the same launch.

Exact relations asserted on top:
  * integer inputs in [-8, 8], integer bias, slope 0.5: EQUAL to float64, hence identical across tiles and splits;
  * systematic residuals: each cross product carries 4e-4 of the outputs that set a channel's maximum (CPU pin);
  * around every split launch: the slabs behind the 64 KiB of counters are NaN before it (an element summed without having been
    written this launch shows), the counters are zero after it, the second launch into the same workspace is bit-identical --
    fp32, planes and scale records byte for byte;
  * the output lives in channels [8, 8 + N) of a buffer 12 channels wider and one image longer: the other channels and the image
    behind the last one keep their sentinels (a fine pixel outside an odd grid would land in a neighbour's row or there);
  * a workspace one byte short of the plan's need, and a null workspace, run unsplit and equal the forced unsplit launch to the
    bit; the short workspace is not touched;
  * fp32 output with a record but no planes: inv = 1, 4 * ptiles * ntn slots, their maximum is max|y|, nothing behind them.

Exclusions -- refused by the library with an error (asserted), nothing else is left out:
  * planes output of the N = 132 shape ("planes output needs N % 32 == 0"): fp32 output with a record instead;
  * the input-gradient role of a layer with 132 coarse channels ("C % 32 == 0").

Measured on the MI355X: worst err / own channel maximum 1.1e-5 with 64-pixel tiles and 1.1e-5 with 128-pixel tiles.  The file's 64
tests run in 3.6 s.
"""
import functools
import time

import numpy as np
import pytest
import torch

import conv_ref as ref
import fx3_col_cases as K
from test_hip_f16x3 import planes_match
from test_hip_f16x3_forms import NAN_BITS, WORST, nchw, per_channel
from test_hip_fp32_plans import SENT, SLOPE, Buf, dev, rnd, spread, with_zeros
from wg3_cases import ints

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_LRELU, EPI_DACT = 0, 1, 2
STASH = {}                 # (case, what) -> bytes of the first plan's exact-integer result
RAN = (b"tconv_ran_tile", b"tconv_ran_cps", b"tconv_ran_split0", b"tconv_ran_split1", b"tconv_ran_split2", b"tconv_ran_split3")


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    t0 = time.time()
    yield functional
    for tile in K.TCONV_TILES:
        if f"tconv {tile}" in WORST:
            print(f"[tconv forms] worst err / own channel maximum, {tile}-pixel tiles: {WORST[f'tconv {tile}']:.2e}")
    print(f"[tconv forms] run time {time.time() - t0:.1f} s")


@pytest.fixture(scope="module")
def lib(F):
    from spatiotemporalentropymodel_amd import _lib
    return _lib.hip()


def ran(lib):
    return tuple(int(lib.stem_tuning_get(k)) for k in RAN)


def bias_of(pre, b):
    return pre if b is None else pre + np.asarray(b, np.float64)[None, :, None, None]


def tconv_operands(name, kind):
    """coarse input [B,C,H,W], weight read as w[c][n][r][s], bias [N] (or None)"""
    B, C, H, W, N, R, oh, ow = K.TCONV_SHAPES[name]
    if kind == "ints":
        return ints((B, C, H, W), 61, 8.0), ints((C, N, R, R), 62, -8.0), ints((N,), 63, -8.0)
    if kind == "resid":
        return (*K.tconv_resid_operands(name), None)
    sn = spread(N)
    return rnd((B, C, H, W), 66), (rnd((C, N, R, R), 67) / np.sqrt(C * R * R / 4)).astype(np.float32) * sn[None, :, None, None], rnd((N,), 68) * sn


@functools.lru_cache(maxsize=None)
def problem(name, kind):
    from spatiotemporalentropymodel_amd import functional as F
    B, C, H, W, N, R, oh, ow = K.TCONV_SHAPES[name]
    Hf, Wf = 2 * H - oh, 2 * W - ow
    x, w, b = tconv_operands(name, kind)
    assert C * R * R * 64 < 2 ** 24
    return dict(name=name, dims=(B, H, W, C, N, R, Hf, Wf), b=b, xp=F.F16Planes.split(dev(x)), wp=F.pack_weight_f16x2_tconv(dev(w)),
                bias=None if b is None else dev(b), pre=ref.conv2d_dx(x, w, (B, N, Hf, Wf), 2, R // 2), z=with_zeros(rnd((B, N, Hf, Wf), 69)))


def launch(F, lib, q, epi, slope, bias, zb, yb, yp, yq, ws_ptr, wsb):
    B, H, W, C, N, R, Hf, Wf = q["dims"]
    xp = q["xp"]
    return lib.stem_tconv2d_f16x3_fwd(xp.data_ptr(), xp.q_ptr(), xp.pix_bytes, q["wp"].data_ptr(), 0 if bias is None else bias.data_ptr(), epi, slope,
                                      0 if zb is None else zb.ptr, 0 if zb is None else zb.ld, 0 if yb is None else yb.ptr, 0 if yb is None else yb.ld,
                                      None if yp is None else yp.data.data_ptr(), yq, B, H, W, C, N, R, Hf, Wf, ws_ptr, wsb, F._stream())


def run_forced(F, lib, q, tile, epi, want, what, split=0, cps=0, slope=SLOPE, bias=None, z=None, out="fp32", ws_mode="own", gate=True, exact=False):
    """one forced tile and plan, launched twice where it splits; ws_mode: "own" (exactly the plan's need), "short" (one byte less:
    unsplit), "null" -> (fp32 output [B,N,Hf,Wf], planes or None, record or None) of the first launch"""
    B, H, W, C, N, R, Hf, Wf = q["dims"]
    M, ntn = B * H * W, K.cdiv(N, K.GBN)
    ns_room = K.tconv_plan(C, R, split=split, cps=cps)[1]
    need = K.tconv_need_bytes(B, H, W, N, ns_room)
    cps_want, ns = K.tconv_plan(C, R, split=split, cps=cps, room=ws_mode == "own")
    splits = max(ns) > 1
    what = f"{what} tile {tile} split {split} cps {cps} ({'/'.join(map(str, ns))})" + ("" if ws_mode == "own" else f" {ws_mode} workspace")
    slots = K.tconv_slots(B, H, W, N, tile)
    zb = None if z is None else Buf(z.shape, N + 8, 4, src=z)
    ws = torch.zeros(need // 4, device="cuda", dtype=torch.int32) if max(ns_room) > 1 and ws_mode != "null" else None
    if ws_mode == "short":
        ws[:] = NAN_BITS                                        # not a workspace the launch may use: it must stay as it is
    outs = []
    with F.tuning(fx3_gen_tile=tile, fx3_split=split, tconv_cps=cps):
        for _ in range(2 if splits else 1):
            if splits:
                ws[K.CNT_BYTES // 4:] = NAN_BITS
            yb = Buf((B + 1, N, Hf, Wf), N + 12, 8)             # one image more than the launch knows of
            yp = rec = None
            if out == "planes":
                yp = F.F16Planes.empty(B, N, Hf, Wf, torch.device("cuda"), min_slots=K.tconv_slots(B, H, W, N, 64))
                yp.data.zero_()
            elif out == "record":
                rec = torch.full((16 + slots + 8,), SENT, device="cuda", dtype=torch.float32)
            rc = launch(F, lib, q, epi, slope, bias, zb, yb, yp, yp.q_ptr() if yp is not None else rec.data_ptr() if rec is not None else None,
                        0 if ws is None else ws.data_ptr(), 0 if ws is None else need - (ws_mode == "short"))
            assert rc == 0, (what, lib.stem_last_error())
            assert ran(lib) == (tile, cps_want, *ns), (what, ran(lib))
            outs.append((yb, yp, rec))
        torch.cuda.synchronize()
    yb, yp, rec = outs[0]
    got = yb.host()[:B]
    if splits:
        assert int(ws[:K.CNT_BYTES // 4].abs().max().item()) == 0, what + ": arrival counters not left at zero"
        assert torch.equal(yb.buf.view(torch.int32), outs[1][0].buf.view(torch.int32)), what + ": second launch into the same workspace differs"
        if yp is not None:
            assert torch.equal(yp.data, outs[1][1].data), what + ": planes / scale record of the second launch differ"
        if rec is not None:
            assert torch.equal(rec.view(torch.int32), outs[1][2].view(torch.int32)), what + ": scale record of the second launch differs"
    if ws_mode == "short":
        assert bool((ws == NAN_BITS).all().item()), what + ": a workspace too small for the plan was used"
    for o in outs:
        assert o[0].others_untouched(), what + ": wrote outside its channel slice"
        assert bool((o[0].view[B:] == SENT).all().item()), what + ": wrote behind the last image"
    assert not np.isnan(got).any(), what + ": NaN in the output (a slab element nobody wrote this launch was summed)"
    if exact:
        assert np.array_equal(got.astype(np.float64), want), f"{what}: {int((got != want).sum())} elements differ from float64, worst {np.abs(got - want).max():.3e}"
        first = STASH.setdefault((q["name"], what.split(" tile ")[0]), got.tobytes())
        assert first == got.tobytes(), what + ": tiles / splits do not agree to the bit"
    elif gate:
        per_channel(got, want, what, f"tconv {tile}")
    if yp is not None:
        if gate and not exact:
            per_channel(nchw(yp.merge()), want, what + " planes", abs_floor=2.0 ** -24 * yp.record()[0])
        assert planes_match(yp, yb.nchw()[:B]), what + ": planes output against the fp32 output of the same launch"
    if rec is not None:
        r = rec.cpu()
        n = int(r[:1].view(torch.int32)[0])
        assert n == slots and float(r[1]) == 1.0 and not r[2:16].any(), (what, n, slots, r[:16])
        assert float(r[16:16 + n].max()) == float(np.abs(got).max()) and bool((r[16 + n:] == SENT).all()), what + ": record's maximum"
    return got, yp, rec


def rich(N):
    return "planes" if N % 32 == 0 else "record"


CASES = [(name, s) for name, (B, C, H, W, N, R, oh, ow) in K.TCONV_SHAPES.items() for s in K.tconv_split_list(C, R)]


@pytest.mark.parametrize("tile", K.TCONV_TILES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-s{c[1]}")
def test_forced_tile_and_split(F, lib, case, tile):
    """forward (bias + leaky ReLU, planes alongside), the input-gradient role (DACT with z from a wider buffer, no bias), bias only
    with a record and no planes; integers exact under bias and slope 0.5; systematic residuals"""
    name, s = case
    N = K.TCONV_SHAPES[name][4]
    p = problem(name, "ints")
    run_forced(F, lib, p, tile, EPI_LRELU, ref.lrelu(bias_of(p["pre"], p["b"]), 0.5), f"{name} integers lrelu 0.5", split=s, slope=0.5, bias=p["bias"],
               out=rich(N), exact=True)
    run_forced(F, lib, p, tile, EPI_DACT, ref.dact(p["pre"], p["z"], 0.5), f"{name} integers dact 0.5", split=s, slope=0.5, z=p["z"], exact=True)
    p = problem(name, "resid")
    run_forced(F, lib, p, tile, EPI_BIAS, p["pre"], f"{name} residuals", split=s)
    p = problem(name, "rand")
    run_forced(F, lib, p, tile, EPI_LRELU, ref.lrelu(bias_of(p["pre"], p["b"]), SLOPE), f"{name} forward", split=s, bias=p["bias"], out=rich(N))
    run_forced(F, lib, p, tile, EPI_DACT, ref.dact(p["pre"], p["z"], SLOPE), f"{name} input gradient", split=s, z=p["z"], out=rich(N))
    run_forced(F, lib, p, tile, EPI_BIAS, bias_of(p["pre"], p["b"]), f"{name} bias only", split=s, bias=p["bias"], out="record")


@pytest.mark.parametrize("tile", K.TCONV_TILES)
@pytest.mark.parametrize("name,cps", [("c64_r5_n132_odd_rows", 5), ("c96_r5_n160_odd_cols", 7), ("c32_r3_n96", 1)])
def test_forced_chunks_per_workgroup(F, lib, name, cps, tile):
    """tconv_cps set directly (fx3_split = 0): the forced value, clamped per phase"""
    B, C, H, W, N, R, oh, ow = K.TCONV_SHAPES[name]
    assert K.tconv_plan(C, R, cps=cps)[0] == cps and max(K.tconv_plan(C, R, cps=cps)[1]) > 1
    p = problem(name, "rand")
    run_forced(F, lib, p, tile, EPI_LRELU, ref.lrelu(bias_of(p["pre"], p["b"]), SLOPE), f"{name} forward", cps=cps, bias=p["bias"], out=rich(N))
    p = problem(name, "ints")
    run_forced(F, lib, p, tile, EPI_LRELU, ref.lrelu(bias_of(p["pre"], p["b"]), 0.5), f"{name} integers lrelu 0.5", cps=cps, slope=0.5, bias=p["bias"], exact=True)


@pytest.mark.parametrize("tile", K.TCONV_TILES)
@pytest.mark.parametrize("name", list(K.TCONV_SHAPES))
def test_workspace_too_small_or_null_runs_unsplit(F, lib, name, tile):
    """the second planning pass: a forced split without room for its slabs (one byte short; no workspace at all) is the forced
    unsplit launch to the bit, and the read-back says so"""
    B, C, H, W, N, R, oh, ow = K.TCONV_SHAPES[name]
    assert max(K.tconv_plan(C, R, split=3)[1]) > 1 and K.tconv_plan(C, R, split=3, room=False) == (K.UNSPLIT_CPS, [1, 1, 1, 1])
    p = problem(name, "rand")
    want = ref.lrelu(bias_of(p["pre"], p["b"]), SLOPE)
    one = run_forced(F, lib, p, tile, EPI_LRELU, want, f"{name} unsplit", split=1, bias=p["bias"], out=rich(N))
    for mode in ("short", "null"):
        got = run_forced(F, lib, p, tile, EPI_LRELU, want, f"{name} forced split", split=3, bias=p["bias"], out=rich(N), ws_mode=mode)
        assert np.array_equal(one[0].view(np.uint32), got[0].view(np.uint32)), f"{name} tile {tile}: a forced split with a {mode} workspace is not the unsplit launch"
        if one[1] is not None:
            assert torch.equal(one[1].data, got[1].data), f"{name} tile {tile}: planes / record with a {mode} workspace"
        else:
            assert torch.equal(one[2].view(torch.int32), got[2].view(torch.int32)), f"{name} tile {tile}: record with a {mode} workspace"
    full = run_forced(F, lib, p, tile, EPI_LRELU, want, f"{name} forced split", split=3, bias=p["bias"], out=rich(N))        # with room it does split
    assert full[0].shape == one[0].shape


def test_refusals(F, lib):
    """N % 32 != 0 has no planes output; a layer with 132 coarse channels has no input-gradient role on this family"""
    p = problem("c64_r5_n132_odd_rows", "rand")
    B, H, W, C, N, R, Hf, Wf = p["dims"]
    yb, yq = Buf((B, N, Hf, Wf), N + 12, 8), torch.zeros(16 + 64, device="cuda")
    assert launch(F, lib, p, EPI_BIAS, SLOPE, p["bias"], None, yb, F.F16Planes.empty(B, 160, Hf, Wf, torch.device("cuda"), min_slots=64), yq.data_ptr(), 0, 0) != 0
    assert b"planes output needs N % 32 == 0" in lib.stem_last_error() and bool((yb.buf == SENT).all().item()) and not bool(yq.any().item())
    q = dict(p, dims=(B, H, W, 132, 64, R, Hf, Wf))
    yb = Buf((B, 64, Hf, Wf))
    assert launch(F, lib, q, EPI_BIAS, SLOPE, None, None, yb, None, None, 0, 0) != 0 and b"C % 32 == 0" in lib.stem_last_error()
    assert bool((yb.buf == SENT).all().item())
    q = dict(p, dims=(B, H, W, C, N, R, Hf - 1, Wf))                 # a fine grid that is neither 2H nor 2H - 1
    assert launch(F, lib, q, EPI_BIAS, SLOPE, None, None, Buf((B, N, Hf - 1, Wf)), None, None, 0, 0) != 0 and b"fine grid" in lib.stem_last_error()


def test_default_planner_keeps_the_64_pixel_tile_for_small_grids(F, lib):
    """nothing forced: every shape of this file is far below 4 * cdiv(M, 128) * ntn >= 256, so the planner never takes the
    128-pixel instantiation here -- which is why it needs the forced runs above"""
    for k in (b"fx3_gen_tile", b"fx3_split", b"tconv_cps"):
        assert lib.stem_tuning_get(k) == 0, k
    for name in K.TCONV_SHAPES:
        p = problem(name, "rand")
        B, H, W, C, N, R, Hf, Wf = p["dims"]
        ws = torch.zeros(int(lib.stem_tconv2d_f16x3_workspace_bytes(B, H, W, C, N, R)) // 4, device="cuda", dtype=torch.int32)
        yb = Buf((B, N, Hf, Wf), N + 12, 8)
        assert launch(F, lib, p, EPI_BIAS, SLOPE, p["bias"], None, yb, None, None, ws.data_ptr(), ws.numel() * 4) == 0, lib.stem_last_error()
        assert ran(lib)[0] == 64 and 4 * K.cdiv(B * H * W, 128) * K.cdiv(N, 128) < 256
        assert int(ws[:K.CNT_BYTES // 4].abs().max().item()) == 0
        per_channel(yb.host(), bias_of(p["pre"], p["b"]), f"{name} default plan", "tconv 64")
