"""numpy references of the three device operations of csrc/resblock.hip (include/stem_blocks.h), forward and backward, in float32 --
every product and sum a single rounding, as the kernels are stated -- and the float64 form of the gate with its error bound.
Arrays are NHWC: x [B, H, W, C].  tests/test_cheng_ref.py pins these on the CPU; tests/test_hip_cheng_ops.py holds the kernels to them.
"""
import numpy as np

F32 = np.float32


def lrelu(v, slope):
    v = np.asarray(v, F32)
    return np.where(v > 0, v, v * F32(slope)).astype(F32)


def pixel_shuffle_fwd(x, r, slope=1.0, addend=None):
    """out[b, h*r+i, w*r+j, c] = act(x[b, h, w, c*r*r + i*r + j]) (+ addend)"""
    B, H, W, Crr = x.shape
    C = Crr // (r * r)
    out = lrelu(x, slope).reshape(B, H, W, C, r, r).transpose(0, 1, 4, 2, 5, 3).reshape(B, H * r, W * r, C)
    if addend is not None:
        out = (out + np.asarray(addend, F32)).astype(F32)
    return np.ascontiguousarray(out)


def pixel_shuffle_bwd(dout, r, x=None, slope=1.0):
    """din[b, h, w, c*r*r + i*r + j] = dout[b, h*r+i, w*r+j, c] * (x > 0 ? 1 : slope); x may be None where slope == 1"""
    B, Ho, Wo, C = dout.shape
    H, W = Ho // r, Wo // r
    d = np.asarray(dout, F32).reshape(B, H, r, W, r, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, H, W, C * r * r)
    if x is not None:
        d = np.where(np.asarray(x, F32) > 0, d, d * F32(slope)).astype(F32)
    return np.ascontiguousarray(d)


def add_act_fwd(a, b, slope=0.0):
    return lrelu((np.asarray(a, F32) + np.asarray(b, F32)).astype(F32), slope)


def add_act_bwd(out, dout, slope=0.0):
    dout = np.asarray(dout, F32)
    return np.where(np.asarray(out, F32) > 0, dout, dout * F32(slope)).astype(F32)


# ---- the gate: out = a * sigmoid(b) + x ------------------------------------------------------------------------------------------
def _sigmoid_pair(b, dtype):
    """(s, 1 - s) the way the kernel forms them: e = exp(-|b|) <= 1, 1 / (1 + e) and e / (1 + e), swapped for b < 0"""
    b = np.asarray(b, dtype)
    e = np.exp(-np.abs(b)).astype(dtype)
    d = (dtype(1) + e).astype(dtype)
    big, small = (dtype(1) / d).astype(dtype), (e / d).astype(dtype)
    return np.where(b >= 0, big, small), np.where(b >= 0, small, big)


def gate_fwd(a, b, x, dtype=F32):
    s, _ = _sigmoid_pair(b, dtype)
    return ((np.asarray(a, dtype) * s).astype(dtype) + np.asarray(x, dtype)).astype(dtype)


def gate_bwd(a, b, dout, dtype=F32):
    """-> (da, db); dx is dout"""
    s, t = _sigmoid_pair(b, dtype)
    dout = np.asarray(dout, dtype)
    da = (dout * s).astype(dtype)
    db = (((dout * np.asarray(a, dtype)).astype(dtype) * s).astype(dtype) * t).astype(dtype)
    return da, db


# Error bound of the fp32 gate against its float64 form on the same fp32 inputs.  u = 2^-24 is the unit roundoff (half an ulp,
# relative); every fp32 +, *, / is correctly rounded: one factor (1 + d), |d| <= u.  The device expf is documented at 1 ulp
# (HIP math API, "expf: maximum ULP error 1"): (1 + d), |d| <= 2u.
#   e  = exp(-|b|)                     2u
#   dd = 1 + e                         the error of e enters with weight e / (1 + e) <= 1/2: u, plus the sum's own u     -> 2u
#   1 / dd                             2u + u                                                                           -> 3u
#   e / dd                             2u (e) + 2u (dd) + u                                                             -> 5u
# so s and 1 - s are each within 5u of sigmoid(b) / 1 - sigmoid(b), at every b (no cancellation, no overflow).  Then
#   out = rn(rn(a s) + x)              |err| <= (5u + u) |a s| + u |a s + x|
#   da  = rn(dout s)                   |err| <= 6u |da|
#   db  = rn(rn(rn(dout a) s) (1-s))   |err| <= (u + 5u + u + 5u + u) |db| = 13u |db|
# to first order; second-order terms (< 20 u^2) are covered by the factor (1 + 2^-10), and results within a factor 2^24 of the
# smallest normal number (where products start to lose bits) by the absolute floor.
U = 2.0 ** -24
GATE_SLACK = 1.0 + 2.0 ** -10
GATE_FLOOR = 2.0 ** -102


def gate_fwd_bound(a, b, x):
    a, b, x = (np.asarray(t, np.float64) for t in (a, b, x))
    p = a / (1.0 + np.exp(-b))
    return GATE_SLACK * U * (6.0 * np.abs(p) + np.abs(p + x)) + GATE_FLOOR


def gate_bwd_bounds(a, b, dout):
    da, db = gate_bwd(a, b, dout, np.float64)
    return GATE_SLACK * 6.0 * U * np.abs(da) + GATE_FLOOR, GATE_SLACK * 13.0 * U * np.abs(db) + GATE_FLOOR
