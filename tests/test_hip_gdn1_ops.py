"""GPU, op level: stem_gdn1_fwd / stem_gdn1_bwd (include/stem_gdn1.h, csrc/gdn1.hip) against tests/gdn1_ref.py in float64.

Shapes: C in {1, 3, 32, 36, 192, 320} (one channel; fewer than one MFMA block; exactly one; one and a partial one with C % 4 == 0 and
C % 32 != 0; the 1080p transform's width; the cap) times npix in {1, 63, 65, 130, CHUNK - 1, CHUNK + 1, 2 CHUNK + 3} (one pixel; the
forward's 64-pixel tile less one and plus one; several tiles with a partial one; the parameter reduction's chunk less one, plus one,
and two chunks with a three-pixel third), CHUNK = STEM_GDN1_PIX_CHUNK.  Every case runs both `inverse` values on dense tensors, on
pitch C + 4 (the 16-byte path where C % 4 == 0) and on the odd pitch 2 C + 5 (the 4-byte path), and compares the three bit for bit.

Inputs: |x[p][j]| = logspace(-2, 1, C)[j] * U(1/2, 1) with random signs, so |x| <= 10 <= 2^7; every 11th element is +0.0 and every
13th -0.0.  Stored gamma = sqrt(U(1/2, 3/2) / C + 2^-36): dense, entries of comparable size, so that one lost k step moves every n
by about 1 / C; every 7th entry lies below the bound 2^-18 (1e-6 or -0.3 in turn).  Stored beta = U(1/2, 3/2), every 5th entry below
sqrt(beta_min + 2^-36) (1e-4 or 0 in turn).

Gates.  Forward: |y - y64| <= (C + 8) 2^-24 |y64| element by element -- C products and C + 1 additions of non-negative terms (no
cancellation), two roundings in gamma', the reciprocal, the product.  Backward: every channel of dx, every row of dgamma, and dbeta
within 1e-4 of their own maximum.  The LowerBound rule entry by entry: a stored value below its bound whose d' is positive gets
exactly 0."""
import numpy as np
import pytest
import torch

import gdn1_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

BETA_MIN = 1e-6


@pytest.fixture(scope="module")
def F():
    from spatiotemporalentropymodel_amd import functional
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return functional


def _chunk():
    from spatiotemporalentropymodel_amd import _lib
    return _lib.header_macro("stem_gdn1.h", "STEM_GDN1_PIX_CHUNK")


CHUNK = _chunk()
CS = (1, 3, 32, 36, 192, 320)
NPIX = (1, 63, 65, 130, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3)


def inputs(C, npix, same_sign=False):
    """-> x, dy [npix, C], beta [C], gamma [C, C] as float32"""
    rng = np.random.default_rng(1000 * C + npix + (7 if same_sign else 0))
    x = (np.logspace(-2, 1, C)[None, :] * rng.uniform(0.5, 1.0, (npix, C))).astype(np.float32)
    dy = rng.uniform(0.5, 1.5, (npix, C)).astype(np.float32)
    if not same_sign:
        x *= rng.choice(np.array([-1.0, 1.0], np.float32), (npix, C))
        dy *= rng.choice(np.array([-1.0, 1.0], np.float32), (npix, C))
        fx = x.reshape(-1)
        fx[5::11] = np.float32(0.0)
        fx[6::13] = np.float32(-0.0)
    gamma = np.sqrt(rng.uniform(0.5, 1.5, (C, C)) / C + ref.PEDESTAL).astype(np.float32)
    fg = gamma.reshape(-1)
    fg[3::14] = np.float32(1e-6)
    fg[10::14] = np.float32(-0.3)
    beta = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta[2::10] = np.float32(1e-4)
    beta[7::10] = np.float32(0.0)
    return x, dy, beta, gamma


def pitched(a, ld):
    """[npix, C] numpy -> [1, C, npix, 1] device tensor with NHWC memory, the first C channels of a NaN-filled buffer ld wide"""
    npix, C = a.shape
    buf = torch.full((1, npix, 1, ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[..., :C] = torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(1, npix, 1, C)
    return buf.permute(0, 3, 1, 2)[:, :C], buf


def out_buffer(npix, C, ld):
    buf = torch.full((1, npix, 1, ld), float("nan"), dtype=torch.float32, device="cuda")
    return buf.permute(0, 3, 1, 2)[:, :C], buf


def rows(buf, C):
    return buf.reshape(-1, buf.shape[-1])[:, :C].cpu().numpy()


def sentinels_intact(buf, C):
    tail = buf.reshape(-1, buf.shape[-1])[:, C:]
    return bool(torch.isnan(tail).all())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run_bwd(F, xv, dyv, beta, gamma, inverse, ld, need_dx=True, need_dp=True, ws_fill=float("nan")):
    """the C entry point itself, so that dx can have a pitch and the workspace a content -> dx rows, dbeta, dgamma (numpy), dx's buffer"""
    from spatiotemporalentropymodel_amd import _lib
    h = _lib.hip()
    _, C, npix, _ = xv.shape
    dxv, dxbuf = out_buffer(npix, C, ld)
    dbeta = torch.full((C,), float("nan"), device="cuda")
    dgamma = torch.full((C, C), float("nan"), device="cuda")
    nbytes = int(h.stem_gdn1_bwd_workspace_bytes(npix, C))
    ws = torch.full((nbytes // 4,), ws_fill, dtype=torch.float32, device="cuda")
    rc = h.stem_gdn1_bwd(xv.data_ptr(), F.nhwc_ld(xv), dyv.data_ptr(), F.nhwc_ld(dyv), beta.data_ptr(), gamma.data_ptr(),
                         dxv.data_ptr() if need_dx else None, ld, dbeta.data_ptr() if need_dp else None,
                         dgamma.data_ptr() if need_dp else None, npix, C, int(inverse), BETA_MIN, ws.data_ptr() if need_dp else None,
                         nbytes if need_dp else 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, h.stem_last_error()
    torch.cuda.synchronize()
    return (rows(dxbuf, C) if need_dx else None, dbeta.cpu().numpy() if need_dp else None, dgamma.cpu().numpy() if need_dp else None, dxbuf)


def gate_forward(y, y64, C, what):
    bound = (C + 8) * 2.0 ** -24 * np.abs(y64)
    err = np.abs(y.astype(np.float64) - y64)
    worst = float((err / np.maximum(np.abs(y64), 1e-300)).max())
    print(f"[gdn1 fwd] {what}: max relative error {worst:.2e}, bound {(C + 8) * 2.0 ** -24:.2e}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements beyond (C + 8) 2^-24 |y|; worst {worst:.3e}"


def gate_rows(a, a64, axis, what, rtol=1e-4):
    """every slice along `axis` within rtol of its own maximum"""
    scale = np.abs(a64).max(axis=axis, keepdims=True)
    err = np.abs(a.astype(np.float64) - a64).max(axis=axis, keepdims=True)
    worst = float((err / np.maximum(scale, 1e-300)).max())
    print(f"[gdn1 bwd] {what}: worst slice {worst:.2e} of its maximum, bound {rtol:.0e}")
    assert (err <= rtol * scale).all(), f"{what}: worst slice is {worst:.3e} of its own maximum (bound {rtol:.0e})"


def gate_lower_bound(stored, d, dprime64, bound, what):
    """below the bound with a clearly positive d': exactly 0; elsewhere the rule passes the gradient (covered by gate_rows)"""
    scale = np.abs(dprime64).max()
    blocked = (stored < bound) & (dprime64 > 1e-3 * scale)
    assert (d[blocked] == 0).all(), f"{what}: {int((d[blocked] != 0).sum())} blocked entries are not exactly 0"
    return int(blocked.sum())


@pytest.mark.parametrize("npix", NPIX)
@pytest.mark.parametrize("C", CS)
def test_forward_backward_against_float64(F, C, npix):
    x, dy, beta, gamma = inputs(C, npix)
    bt, gt = torch.from_numpy(beta).cuda(), torch.from_numpy(gamma).cuda()
    nblocked = 0
    for inverse in (False, True):
        y64 = ref.forward(x, beta, gamma, inverse, BETA_MIN)
        dx64, db64, dg64, dbp64, dgp64 = ref.backward(x, dy, beta, gamma, inverse, BETA_MIN)
        first = None
        for ld in (C, C + 4, 2 * C + 5):
            what = f"C={C} npix={npix} inverse={inverse} ld={ld}"
            xv, _ = pitched(x, ld)
            dyv, _ = pitched(dy, ld)
            yv, ybuf = out_buffer(npix, C, ld)
            F.gdn1_forward(xv, bt, gt, inverse, BETA_MIN, out=yv)
            dx, db, dg, dxbuf = run_bwd(F, xv, dyv, bt, gt, inverse, ld)
            y = rows(ybuf, C)
            assert sentinels_intact(ybuf, C) and sentinels_intact(dxbuf, C), f"{what}: wrote past channel C of a pixel"
            if first is None:
                first = (y, dx, db, dg)
                gate_forward(y, y64, C, what)
                gate_rows(dx, dx64, 0, what + " dx")
                gate_rows(dg, dg64, 1, what + " dgamma")
                gate_rows(db[None, :], db64[None, :], 1, what + " dbeta")
                nblocked += gate_lower_bound(gamma, dg, dgp64, ref.GAMMA_BOUND, what + " dgamma")
                nblocked += gate_lower_bound(beta, db, dbp64, ref.beta_bound(BETA_MIN), what + " dbeta")
            else:
                for a, b, name in zip(first, (y, dx, db, dg), ("y", "dx", "dbeta", "dgamma")):
                    assert np.array_equal(bits(a), bits(b)), f"{what}: {name} differs from the dense run's bits"
    if C >= 32:
        assert nblocked > 0, "no entry exercised the blocking side of the LowerBound rule"


@pytest.mark.parametrize("C,npix", [(36, 130), (192, CHUNK + 1), (320, 2 * CHUNK - 1)])
def test_same_sign_sums_lose_no_pixel(F, C, npix):
    """x > 0 and dy >= 0: every term of dgamma' and dbeta' has one sign, so a lost pixel moves every entry by at least 1 / npix > 1e-4"""
    assert npix <= 2048
    x, dy, beta, gamma = inputs(C, npix, same_sign=True)
    assert (x > 0).all() and (dy >= 0).all()
    bt, gt = torch.from_numpy(beta).cuda(), torch.from_numpy(gamma).cuda()
    for inverse in (False, True):
        dx64, db64, dg64, _, _ = ref.backward(x, dy, beta, gamma, inverse, BETA_MIN)
        xv, _ = pitched(x, C)
        dyv, _ = pitched(dy, C)
        dx, db, dg, _ = run_bwd(F, xv, dyv, bt, gt, inverse, C)
        what = f"same sign C={C} npix={npix} inverse={inverse}"
        gate_rows(dx, dx64, 0, what + " dx")
        gate_rows(dg, dg64, 1, what + " dgamma")
        gate_rows(db[None, :], db64[None, :], 1, what + " dbeta")


@pytest.mark.parametrize("C,npix", [(3, 130), (36, CHUNK + 1), (192, 2 * CHUNK + 3), (320, 65)])
def test_bits_do_not_depend_on_launch_workspace_position_or_request(F, C, npix):
    x, dy, beta, gamma = inputs(C, npix)
    bt, gt = torch.from_numpy(beta).cuda(), torch.from_numpy(gamma).cuda()
    perm = np.random.default_rng(C + npix).permutation(npix)
    for inverse in (False, True):
        xv, _ = pitched(x, C)
        dyv, _ = pitched(dy, C)
        y = rows(F.gdn1_forward(xv, bt, gt, inverse, BETA_MIN).permute(0, 2, 3, 1).contiguous(), C)
        dx, db, dg, _ = run_bwd(F, xv, dyv, bt, gt, inverse, C, ws_fill=float("nan"))
        # repeated launches, and a zeroed workspace against the NaN-poisoned one
        dx2, db2, dg2, _ = run_bwd(F, xv, dyv, bt, gt, inverse, C, ws_fill=0.0)
        for a, b, name in ((dx, dx2, "dx"), (db, db2, "dbeta"), (dg, dg2, "dgamma")):
            assert np.array_equal(bits(a), bits(b)), f"{name}: a second launch on a zeroed workspace gave other bits"
        assert np.isfinite(db).all() and np.isfinite(dg).all()
        assert np.array_equal(bits(y), bits(rows(F.gdn1_forward(xv, bt, gt, inverse, BETA_MIN).permute(0, 2, 3, 1).contiguous(), C)))
        # pixels permuted on input against outputs permuted the same way
        xp, _ = pitched(x[perm], C)
        dyp, _ = pitched(dy[perm], C)
        yp = rows(F.gdn1_forward(xp, bt, gt, inverse, BETA_MIN).permute(0, 2, 3, 1).contiguous(), C)
        dxp, _, _, _ = run_bwd(F, xp, dyp, bt, gt, inverse, C, need_dp=False)
        assert np.array_equal(bits(yp), bits(y[perm])), "y depends on where a pixel sits"
        assert np.array_equal(bits(dxp), bits(dx[perm])), "dx depends on where a pixel sits"
        # what is asked for does not change what is computed (functional.gdn1_backward, which allocates its own workspace)
        only_dx = F.gdn1_backward(xv, dyv, bt, gt, inverse, BETA_MIN, need_dx=True, need_dparams=False)
        only_dp = F.gdn1_backward(xv, dyv, bt, gt, inverse, BETA_MIN, need_dx=False, need_dparams=True)
        assert only_dx[1] is None and only_dx[2] is None and only_dp[0] is None
        assert np.array_equal(bits(rows(only_dx[0].permute(0, 2, 3, 1).contiguous(), C)), bits(dx))
        assert np.array_equal(bits(only_dp[1].cpu().numpy()), bits(db)) and np.array_equal(bits(only_dp[2].cpu().numpy()), bits(dg))


def test_refusals_on_the_device(F):
    """the Python veneer: a channel count beyond the cap and parameters of another width are refused; nothing asked for is an error"""
    cap = F.GDN1_MAX_C
    x = F.empty_nhwc(1, cap + 4, 2, 2, "cuda")
    with pytest.raises(RuntimeError, match="stem_gdn1_fwd"):
        F.gdn1_forward(x, torch.ones(cap + 4, device="cuda"), torch.ones(cap + 4, cap + 4, device="cuda"))
    x = F.empty_nhwc(1, 8, 2, 2, "cuda")
    with pytest.raises(ValueError, match="gdn1_forward"):
        F.gdn1_forward(x, torch.ones(4, device="cuda"), torch.ones(8, 8, device="cuda"))
    with pytest.raises(ValueError, match="nothing to compute"):
        F.gdn1_backward(x, x, torch.ones(8, device="cuda"), torch.ones(8, 8, device="cuda"), False, 1e-6, need_dx=False, need_dparams=False)
