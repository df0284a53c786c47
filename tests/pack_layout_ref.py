"""Plain numpy references for the weight pack, slab-sum, bias-gradient and layout kernels (csrc/pack.hip, the tail of csrc/wgrad.hip,
stem_amax_nhwc), and the case lists both test files iterate over.

No torch, no GPU and nothing of the package's native code: tests/test_pack_layout_ref.py pins these functions on the CPU (index
identities of include/stem_hip.h, a masked convolution against torch in float64, a-priori rounding bounds) and checks the
preconditions of the GPU gates; tests/test_hip_pack_layout.py compares the HIP kernels with them, bit for bit.

  pack_ref                          the five roles of stem_pack_weight, masks included -> (packed copy, weight as it is left)
  unpack_exact / unpack_f32         sum over the split-K slabs in the reference layout: float64, and float32 in the documented order
                                    (even slabs into one accumulator, odd slabs into another, both from 0, result even + odd)
  colsum_final_f32                  second stage of the bias gradient in the order of colsum_final_kernel
  nchw_to_nhwc / nhwc_to_nchw       the layout kernels; nhwc4_with_record / amax_record_max: the scale record of stem_common.h
  dyadic / cancelling               the two input generators: sums that are exact in fp32 in any order / sums whose rounding
                                    depends on the order
"""
import numpy as np

PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_DECONV_FWD, PACK_DECONV_DGRAD, PACK_CONV_FWD_C4 = 0, 1, 2, 3, 4
MASK_B = 4                                # bit 2 of `masked`: type B; bits 0-1: mode (1 = packed copy only, 2 = the weight too)
UNPACK_DECONV, UNPACK_ACCUMULATE = 1, 2
QREC_HDR = 16                             # floats in front of the slots of a scale record
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ pack
def mask_taps(R, S, masked):
    """[R,S] bool: the taps a MaskedConv2d zeroes -- row > R/2, or row == R/2 and col >= S/2 (+ 1 for type B)"""
    r, s = np.meshgrid(np.arange(R), np.arange(S), indexing="ij")
    return (r > R // 2) | ((r == R // 2) & (s >= S // 2 + ((masked >> 2) & 1)))


def pack_ref(w, role, masked=0):
    """w: Conv2d [K,C,R,S] (roles CONV_FWD, CONV_DGRAD, CONV_FWD_C4) or ConvTranspose2d [C,K,R,S] (DECONV_FWD, DECONV_DGRAD)
    -> (packed, w_after): [R*S][K][C] for the FWD roles, [R*S][C][K] for the DGRAD roles, [K][32][4] zero padded for C4.
    masked & 3 = 1 zeroes the masked taps in the packed copy, = 2 in the weight as well; C4 takes no mask."""
    w = np.asarray(w)
    R, S = w.shape[2:]
    T = R * S
    if role == PACK_CONV_FWD_C4:
        K, C = w.shape[:2]
        assert C <= 4 and T <= 32 and not masked
        out = np.zeros((K, 32, 4), w.dtype)
        out[:, :T, :C] = w.reshape(K, C, T).transpose(0, 2, 1)
        return out, w.copy()
    after = w.copy()
    src = w.copy()
    if masked & 3:
        src[:, :, mask_taps(R, S, masked)] = 0
        if (masked & 3) == 2:
            after = src.copy()
    flat = src.reshape(w.shape[0], w.shape[1], T)                # [d0][d1][t]
    # Conv2d: d0 = K, d1 = C.  ConvTranspose2d: d0 = C, d1 = K.  FWD wants [t][K][C], DGRAD [t][C][K].
    d0_first = role in (PACK_CONV_FWD, PACK_DECONV_DGRAD)
    assert role in (PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_DECONV_FWD, PACK_DECONV_DGRAD), role
    out = flat.transpose(2, 0, 1) if d0_first else flat.transpose(2, 1, 0)
    return np.ascontiguousarray(out), after


def pack_shape(K, C, R, S, role):
    """shape of the torch weight a (K, C, R, S, role) case packs"""
    return (C, K, R, S) if role in (PACK_DECONV_FWD, PACK_DECONV_DGRAD) else (K, C, R, S)


# ------------------------------------------------------------------------------------------------------------------ slab sums
def _slabs(slabs, K, C, R, S, deconv):
    """[splits][T][A][Bd] with (A, Bd) = (K, C) for Conv2d, (C, K) for ConvTranspose2d"""
    A, Bd = (C, K) if deconv else (K, C)
    slabs = np.asarray(slabs)
    return slabs.reshape(-1, R * S, A, Bd), (A, Bd, R, S)


def unpack_exact(slabs, K, C, R, S, deconv=False):
    """float64 sum over the slabs, in the reference layout: Conv2d [K,C,R,S] from slabs [t][K][C], ConvTranspose2d [C,K,R,S]
    from slabs [t][C][K]"""
    x, shape = _slabs(slabs, K, C, R, S, deconv)
    return x.astype(np.float64).sum(0).transpose(1, 2, 0).reshape(shape)


def unpack_f32(slabs, K, C, R, S, deconv=False, old=None):
    """the same sum in float32 in the order unpack_kernel and both routes of unpack_multi_kernel document: v0 = 0 + slab 0 + slab 2
    + ..., v1 = 0 + slab 1 + slab 3 + ..., result v0 + v1; with ACCUMULATE (`old` given) old + result, one more rounding"""
    x, shape = _slabs(slabs, K, C, R, S, deconv)
    x = x.astype(np.float32)
    v0, v1 = np.zeros(x.shape[1:], np.float32), np.zeros(x.shape[1:], np.float32)
    for s in range(0, x.shape[0], 2):
        v0 = v0 + x[s]
    for s in range(1, x.shape[0], 2):
        v1 = v1 + x[s]
    v = (v0 + v1).transpose(1, 2, 0).reshape(shape)
    return v if old is None else (np.asarray(old, np.float32).reshape(shape) + v)


def unpack_sequential_f32(slabs, K, C, R, S, deconv=False):
    """the plain sequential float32 sum ((s0 + s1) + s2) + ...: NOT what the kernels do -- the order-sensitivity precondition
    compares unpack_f32 with it"""
    x, shape = _slabs(slabs, K, C, R, S, deconv)
    v = np.zeros(x.shape[1:], np.float32)
    for s in range(x.shape[0]):
        v = v + x[s].astype(np.float32)
    return v.transpose(1, 2, 0).reshape(shape)


# ------------------------------------------------------------------------------------------------------------------ bias gradient
def colsum_final_f32(part, accumulate_into=None):
    """part [parts][K] -> [K] in the order of colsum_final_kernel: row group r = 0..15 sums parts r, r + 16, r + 32, ... sequentially
    from 0, the 16 group sums are added in order from 0; accumulate_into: old + that, one more rounding"""
    part = np.asarray(part, np.float32)
    v = np.zeros(part.shape[1], np.float32)
    for r in range(16):
        s = np.zeros(part.shape[1], np.float32)
        for p in range(r, part.shape[0], 16):
            s = s + part[p]
        v = v + s
    return v if accumulate_into is None else (np.asarray(accumulate_into, np.float32) + v)


def colsum_sequential_f32(part):
    """plain sequential float32 column sum (the comparison of the order-sensitivity precondition)"""
    part = np.asarray(part, np.float32)
    v = np.zeros(part.shape[1], np.float32)
    for p in range(part.shape[0]):
        v = v + part[p]
    return v


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-24: |fl(sum of n terms, any order) - exact| <= gamma_(n-1) sum |x| (Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2); the tests use gamma_n with n = number of summed terms (+ 1 for ACCUMULATE)"""
    return n * U24 / (1.0 - n * U24)


# ------------------------------------------------------------------------------------------------------------------ layouts
def nchw_to_nhwc(x):
    """[B,C,H,W] -> [B,H,W,C]"""
    return np.ascontiguousarray(np.asarray(x).transpose(0, 2, 3, 1))


def nhwc_to_nchw(x, clamp01=False):
    """[B,H,W,C] -> [B,C,H,W]; clamp01: min(max(v, 0), 1)"""
    y = np.ascontiguousarray(np.asarray(x).transpose(0, 3, 1, 2))
    return np.minimum(np.maximum(y, np.float32(0)), np.float32(1)) if clamp01 else y


def nhwc4_with_record(x):
    """x [B,3,H,W] fp32 -> (y [B,H,W,4] with a zero fourth component, record): the record (stem_common.h) is QREC_HDR + nslots
    floats -- word 0 the int slot count, word 1 the float 1.0, words 2..15 zero, slot j = max |x| over the pixels
    [1024 j, 1024 (j + 1)) of the flattened B*H*W, nslots = ceil(B*H*W / 1024)"""
    x = np.asarray(x, np.float32)
    B, C, H, W = x.shape
    assert C == 3
    y = np.zeros((B, H, W, 4), np.float32)
    y[..., :3] = x.transpose(0, 2, 3, 1)
    pix = np.abs(y.reshape(-1, 4)).max(1)
    ns = (pix.size + 1023) // 1024
    q = np.zeros(QREC_HDR + ns, np.float32)
    q[:1].view(np.int32)[0] = ns
    q[1] = 1.0
    for j in range(ns):
        q[QREC_HDR + j] = pix[1024 * j:1024 * (j + 1)].max()
    return y, q


def amax_record_max(q):
    """a scale record -> (slot count, maximum over its slots)"""
    q = np.asarray(q, np.float32)
    ns = int(q[:1].view(np.int32)[0])
    assert 0 < ns <= q.size - QREC_HDR, ns
    return ns, float(q[QREC_HDR:QREC_HDR + ns].max())


def amax_slots(npix, C, max_slots):
    """the slot count stem_amax_nhwc uses: one workgroup per 2048 float4 pieces, at least 1, at most max_slots and 1024"""
    return int(min(max((npix * (C // 4) + 2047) // 2048, 1), max_slots, 1024))


# ------------------------------------------------------------------------------------------------------------------ inputs
DYADIC_MAX, DYADIC_STEP = 8.0, 2.0 ** -3


def dyadic(shape, seed):
    """fp32 values on the grid of 2^-3 in [-8, 8]: a sum of n of them is an integer multiple of 2^-3 of magnitude <= 8 n, exact in
    fp32 in ANY order as long as 8 n * 8 < 2^24 (n < 2^18) -- the GPU result must equal the integer sum bit for bit"""
    return (np.random.default_rng(seed).integers(-64, 65, shape) * DYADIC_STEP).astype(np.float32)


def dyadic_is_exact(nterms):
    """the precondition of every exact gate on `dyadic` inputs: max partial |sum| * 8 < 2^24"""
    return nterms * DYADIC_MAX * 8 < 2 ** 24


def cancelling(shape, seed):
    """fp32 values of mixed sign whose magnitudes 10^u, u uniform in [-2, 2], spread over four decades along every axis, the
    summed (first) one included: the rounded float32 sum depends on the order of the additions"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-2.0, 2.0, shape)).astype(np.float32)


def case_seed(*fields):
    """a deterministic seed from a case's integer fields"""
    s = 0x9E3779B9
    for f in fields:
        s = (s * 1000003 + int(f) + 1) % (1 << 31)
    return s


# ------------------------------------------------------------------------------------------------------------------ case lists
# ---- pack: (K, C, R, S)
PACK_SHAPES = [(5, 3, 5, 5), (96, 64, 3, 3), (7, 385, 3, 3), (128, 96, 1, 1), (6, 10, 2, 3), (10, 6, 3, 2)]
PACK_ROLES = [PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_DECONV_FWD, PACK_DECONV_DGRAD]
PACK_C4_CASES = [(6, 3, 5, 5), (6, 4, 5, 5), (64, 3, 3, 3), (5, 4, 3, 3)]
PACK_MASKS = [1, 2, 1 | MASK_B, 2 | MASK_B]
PACK_MASKED_SHAPES = [(10, 6, 5, 5), (6, 10, 3, 3), (6, 10, 2, 3), (3, 5, 3, 2)]
PACK_LDS_BIG = (2, 672, 5, 5, PACK_CONV_FWD, 2)            # Bd * T * 4 = 67200 B > 64 KiB: the dynamic-LDS attribute branch
PACK_LDS_OVER = (1, 1700, 5, 5, PACK_CONV_FWD, 0)          # 170000 B > 160 KiB: an error, nothing launched


def _pack_multi_cases():
    """33 descriptors (K, C, R, S, role, masked): the table is split at 32.  Roles, tap counts and masks mixed, the > 64 KiB case
    in the first launch, a mode-2 mask in the second"""
    cases = [(K, C, R, S, role, 0) for i, (K, C, R, S) in enumerate(PACK_SHAPES) for role in PACK_ROLES if (i + role) % 2 == 0]      # 12
    cases += [s + (PACK_ROLES[i % 4], PACK_MASKS[(i + j) % 4]) for i, s in enumerate(PACK_MASKED_SHAPES) for j in range(4)]         # 16
    cases += [PACK_LDS_BIG, (5, 3, 5, 5, PACK_DECONV_FWD, 0), (7, 385, 3, 3, PACK_CONV_DGRAD, 1), (6, 10, 2, 3, PACK_DECONV_DGRAD, 0)]
    cases += [(10, 6, 5, 5, PACK_CONV_DGRAD, 2 | MASK_B)]
    assert len(cases) == 33
    return cases


PACK_MULTI_CASES = _pack_multi_cases()

# ---- slab sum: (A, Bd, T, splits, deconv); K, C, R, S through unpack_kcrs
TAPS = {1: (1, 1), 4: (2, 2), 6: (2, 3), 9: (3, 3), 25: (5, 5)}
UNPACK_CASES = [
    (5, 3, 25, 1, False), (4, 32, 9, 2, False), (3, 37, 6, 3, True), (6, 64, 4, 4, False),
    (3, 100, 9, 5, False),                       # Bd = 100: ranges of 64 -> a full one (float4 route) and one of 36 (scalar route)
    (2, 385, 1, 7, True), (2, 64, 25, 8, True), (7, 100, 1, 7, False), (3, 64, 9, 3, False), (5, 37, 25, 8, False),
    (2, 385, 4, 5, False), (3, 32, 6, 4, True), (1, 128, 9, 7, False), (2, 192, 4, 8, True), (4, 3, 1, 2, True),
    (1, 100, 25, 3, False), (2, 64, 6, 1, False), (2, 64, 1, 2, True),
    # the automatic run length: 192, 160, 128, 96 (the longest that divides Bd and leaves A * Bd / mb >= 512 workgroups)
    (512, 192, 1, 8, False), (512, 320, 1, 8, True), (512, 128, 1, 3, False), (512, 96, 1, 5, True),
]
UNPACK_AUTO_MB = {(512, 192): 192, (512, 320): 160, (512, 128): 128, (512, 96): 96}
UNPACK_MB_VALUES = [0, 32, 64, 96, 128, 160, 192]
UNPACK_MISALIGNED_CASES = [(6, 64, 4, 4, False), (3, 100, 9, 5, False), (2, 64, 25, 8, True), (512, 128, 1, 3, False)]


def unpack_kcrs(case):
    A, Bd, T, splits, deconv = case
    R, S = TAPS[T]
    return ((Bd, A) if deconv else (A, Bd)) + (R, S)


def unpack_auto_mb(A, Bd):
    """the run length stem_unpack_wgrads_multi picks on its own"""
    for mb in range(192, 64, -32):
        if Bd % mb == 0 and A * (Bd // mb) >= 512:
            return mb
    return 64


def unpack_slabs(case, kind, salt=0):
    """the slabs [splits][T][A][Bd] of a case: kind "dyadic" or "cancelling" """
    A, Bd, T, splits, deconv = case
    gen = dyadic if kind == "dyadic" else cancelling
    return gen((splits, T, A, Bd), case_seed(A, Bd, T, splits, int(deconv), salt))


def order_sensitive_slabs(splits):
    """with one or two slabs there is only one order (0 + s0 [+ s1]); from three on the documented order differs from the sequential one"""
    return splits >= 3


def _unpack_table_cases():
    """33 descriptors (case, flags beyond DECONV, misaligned dw): the table is split at 32"""
    small = [c for c in UNPACK_CASES if c[0] < 512]
    out = [(small[i % len(small)], UNPACK_ACCUMULATE if i % 3 == 1 else 0, i % 5 == 2) for i in range(31)]
    out.insert(7, (UNPACK_CASES[-2], 0, False))
    out.append((UNPACK_CASES[-1], UNPACK_ACCUMULATE, False))
    assert len(out) == 33
    return out


UNPACK_TABLE_CASES = _unpack_table_cases()

# ---- bias gradient, second stage: (parts, K)
BIAS_FINAL_PARTS = [1, 15, 16, 17, 33, 512]
BIAS_FINAL_K = [1, 63, 64, 65, 192, 385]
BIAS_FINAL_CASES = [(p, k) for p in BIAS_FINAL_PARTS for k in BIAS_FINAL_K]
BIAS_FINAL_SALT = 3                       # chosen so that the one-element cases (K = 1, parts > 16) are order sensitive too
# 25 descriptors (parts, K, accumulate) = two launches (24 + 1); the widest (K = 385) sits next to K = 1 and K = 63
BIAS_FINAL_MULTI = [(17, 63, 0), (33, 385, 1), (512, 1, 0)] + [(p, k, (i + j) % 2) for i, p in enumerate([1, 15, 16, 17, 33, 512])
                                                               for j, k in enumerate([1, 64, 65, 192])][:21] + [(33, 63, 1)]
assert len(BIAS_FINAL_MULTI) == 25


def order_sensitive_parts(parts):
    """up to 16 parts every row group holds at most one part and the 16 group sums are added in order: the sequential sum"""
    return parts > 16


def bias_final_parts(case, kind):
    parts, K = case
    gen = dyadic if kind == "dyadic" else cancelling
    return gen((parts, K), case_seed(parts, K, BIAS_FINAL_SALT))


# ---- bias gradient from dy: (npix, K, pitch kind)
BIAS_PITCHES = ["dense", "pad4", "odd", "slice1"]
BIAS_NPIX = [1, 127, 128, 129, 1000, 5000]
BIAS_K = [1, 3, 4, 60, 64, 68, 385]


def bias_pitch(K, kind):
    """-> (ld, first channel): ld = K; ld > K with ld % 4 == 0; ld > K with ld % 4 != 0; channels 1 .. K + 1 of a buffer whose width is
    a multiple of 4 (aligned shape, base 4 bytes off a 16-byte boundary)"""
    if kind == "dense":
        return K, 0
    if kind == "pad4":
        return (K // 4 + 2) * 4, 0
    if kind == "odd":
        return (K // 4 + 1) * 4 + 1, 0
    return (K // 4 + 2) * 4, 1


def _bias_grad_cases():
    cases, i = [], 0
    for K in BIAS_K:
        for kind in BIAS_PITCHES:
            npixs = BIAS_NPIX[:4] if K == 385 else BIAS_NPIX            # K = 385 stays small
            cases.append((npixs[i % len(npixs)], K, kind))
            i += 1
    cases += [(5000, 64, kind) for kind in BIAS_PITCHES if (5000, 64, kind) not in cases]      # 40 parts: more than the 16 row groups
    cases += [(1000, 68, "dense"), (129, 4, "pad4"), (127, 60, "dense"), (128, 64, "pad4")]   # float4 route: tail only, one unrolled pass
    return cases


BIAS_GRAD_CASES = _bias_grad_cases()
BIAS_GRAD_CANCELLING = (5000, 64, "dense")


def bias_parts(npix, K):
    """the part count of the first stage (colsum_parts): about 1536 workgroups, at least 128 rows per part, at most 512 parts"""
    return int(max(1, min(1536 // ((K + 63) // 64), (npix + 127) // 128, 512)))


# ---- layouts
TRANSPOSE_CASES = [(3, 37, 9, 11), (1, 1, 1, 1), (2, 33, 1, 31), (2, 64, 32, 32)]          # (B, C, H, W): HW = 99, 1, 31, 1024
CLAMP_VALUES = np.array([-1.0, -0.0, 0.0, 1e-30, -1e-30, 0.5, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 2.0, 3e38, -3e38,
                         np.inf, -np.inf], np.float32)
COPY_CHANNELS_C = [1, 37, 96]
NHWC4_CASES = [(1, 1, 1), (1, 15, 17), (1, 32, 32), (1, 25, 41), (3, 20, 35)]             # (B, H, W): 1, 255, 1024, 1025, 2100 pixels
AMAX_CASES = [(npix, C, ms) for npix in (1, 2047, 2049, 70000) for C in (4, 32, 100) for ms in (3, 2000)
              if not (npix == 1 and ms == 3)] + [(1, 4, 1), (2049, 100, 1)]
