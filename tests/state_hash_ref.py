"""The conditioning-state hash of the sequence codecs in numpy (include/stem_statehash.h states the definition; csrc/statehash.hip is
the kernel).  For image b of x [B,C,H,W] fp32:

    out[b] = sum over (c, h, w) of mix64((i << 32) | bits(x[b,c,h,w]))  mod 2^64,    i = (c * H + h) * W + w

with mix64 the SplitMix64 output function.  The index is the LOGICAL one: numpy's reshape(-1) of a view walks it in that order whatever
the strides are, so the memory layout never enters.  `state_hash_int` is the same thing in Python integers, one element at a time."""
import struct

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
M1 = 0xBF58476D1CE4E5B9
M2 = 0x94D049BB133111EB

#: the known answers of the issue that introduced the hash: (values, shape [C,H,W], hash)
KNOWN = (([0.0], (1, 1, 1), 0xE220A8397B1DCDAF),
         ([-0.0], (1, 1, 1), 0x25493CC63225736C),
         ([0.0, 1.0], (2, 1, 1), 0xB38B8E662B7BF540),
         ([1.0, 0.0], (1, 1, 2), 0xC195B436145E136D),
         ([0.0, 1.0, 2.0, 3.0, 4.0, 5.0], (2, 1, 3), 0x69EE030164F69B13))


def mix64(k):
    """SplitMix64's output function on a uint64 array (arithmetic mod 2^64: numpy's unsigned wrap-around)"""
    with np.errstate(over="ignore"):
        z = k + np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
        return z ^ (z >> np.uint64(31))


def terms(bits, first=0):
    """the terms of the elements with logical indexes first .. first + len(bits) and bit patterns `bits` (uint32), as uint64"""
    bits = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
    i = np.arange(first, first + bits.size, dtype=np.uint64)
    return mix64((i << np.uint64(32)) | bits.astype(np.uint64))


def state_hash(x):
    """x: a float32 array [B,C,H,W] with any strides -> a list of B Python ints in [0, 2^64)"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4, (x.dtype, x.shape)
    out = []
    for b in range(x.shape[0]):
        bits = np.ascontiguousarray(x[b]).reshape(-1).view(np.uint32)
        with np.errstate(over="ignore"):
            out.append(int(np.sum(terms(bits), dtype=np.uint64)))
    return out


def mix64_int(k):
    z = (k + GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * M1) & MASK
    z = ((z ^ (z >> 27)) * M2) & MASK
    return z ^ (z >> 31)


def state_hash_int(x):
    """the same in Python integers: no array arithmetic, every element's bits through struct"""
    x = np.asarray(x)
    B, C, H, W = x.shape
    out = []
    for b in range(B):
        total = 0
        for c in range(C):
            for h in range(H):
                for w in range(W):
                    bits = struct.unpack("<I", struct.pack("<f", x[b, c, h, w]))[0] if not np.isnan(x[b, c, h, w]) else int(
                        x[b:b + 1, c, h, w].view(np.uint32)[0])               # struct may canonicalise a NaN: read its bits directly
                    total += mix64_int((((c * H + h) * W + w) << 32) | bits)
        out.append(total & MASK)
    return out
