"""Writes tests/golden/yuv_transforms*.npz: what the reference's own colour transforms (compressai/transforms/functional.py,
loaded by path: it needs only torch) give on seeded inputs, in float32 and float64, for tests/test_yuv_abi.py and
tests/test_hip_yuv.py.  Run on the CPU, by hand, with the reference tree at hand; not part of the test run.

    python tests/golden/make_golden_yuv.py /path/to/reference

Per case "<H>x<W>_<bits>" (B images):
    y, u, v                     seeded integer planes, uniform over 0 .. 2^bits - 1 (uint8 / uint16)
    rgb32_<mode>, rgb64_<mode>  ycbcr2rgb(yuv_420_to_444(planes / peak, mode)), mode = bilinear | nearest          [B,3,H,W]
    src                         seeded RGB, uniform in [0,1), float32                                              [B,3,H,W]
    y32, u32, v32, y64, u64, v64   yuv_444_to_420(rgb2ycbcr(src))                                                   [B,H,W] / [B,H/2,W/2]
The float64 runs take the same inputs converted to float64.  The reference passes align_corners=False to F.interpolate for
"nearest" too, which torch refuses; that one call is made here without the argument (it has no meaning for "nearest").

Shapes: 2x2 (every tap clamps), 4x6, 34x70 and 66x258 with B = 3 (no multiple of 32 or 64, one chroma sample past a power of
two), 4x1026 (one chroma sample more, each way, than the 2 x 1024 strip a workgroup of csrc/yuv.hip covers; W % 4 == 2: the
element-wise path) and 4x1028 with B = 2 (the same on the vector path, W % 4 == 0); 8 and 10 bits, except 66x258 (8 bits only).

Size.  Dense float32 + float64 images of random inputs cost about 100 bytes per pixel that no compressor shortens.  To bound that:
the inputs (planes, src) are kept for all B images, which is what the squared-error and round-trip tests need, but from 34x70
upwards the float results are kept for the LAST image only (`ref_images`: a wrong batch stride still shows there), and the float32
copies, the yardstick of the gate and of the host transforms, only up to 34x70 (F32_MAX_PIXELS).  Every array is stored image by
image ("<case>/<name>/<b>") in part files of at most PART_BYTES (no committed file may exceed 1 MiB): yuv_transforms.npz, then
yuv_transforms.1.npz, ...; tests/yuv_fixture.py puts them together again.

The generator also checks what the tests assert about the inputs: the reference's float32 results lie within 2e-6 of its float64
ones, and quantising its float32 planes disagrees with rint() of the float64 ones on at most 0.1 % of a case's samples.
"""
import glob
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEM = os.path.join(HERE, "yuv_transforms")
PART_BYTES = 900 * 1024
CASES = [(2, 2, 1), (4, 6, 2), (34, 70, 3), (66, 258, 3), (4, 1026, 1), (4, 1028, 2)]         # H, W, B
BITS = (8, 10)
SKIP = {(66, 258, 10)}
GATE = 2e-6
EXCUSED_SHARE = 1e-3
ALL_IMAGES_MAX_PIXELS = 100            # H * W up to which the float results of every image are kept
F32_MAX_PIXELS = 34 * 70               # H * W up to which the float32 results are kept


def case_names():
    return [(f"{H}x{W}_{bits}", H, W, B, bits) for H, W, B in CASES for bits in BITS if (H, W, bits) not in SKIP]


def quantise(v, peak):
    return np.rint(np.clip(v, 0.0, 1.0) * peak)


def main(reference):
    import torch
    import torch.nn.functional as F
    spec = importlib.util.spec_from_file_location("ref_transforms_functional", os.path.join(reference, "compressai", "transforms", "functional.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    def to_444(planes, mode):
        if mode == "bilinear":
            return ref.yuv_420_to_444(planes, mode=mode)
        y, u, v = planes                                   # the reference's call, minus the argument torch refuses for "nearest"
        return torch.cat((y, F.interpolate(u, scale_factor=2, mode=mode), F.interpolate(v, scale_factor=2, mode=mode)), dim=1)

    members = {}
    for seed, (case, H, W, B, bits) in enumerate(case_names()):
        rng = np.random.default_rng(20261018 + seed)
        peak = (1 << bits) - 1
        dt = np.uint8 if bits == 8 else np.uint16
        planes = [rng.integers(0, peak + 1, size=s, dtype=dt) for s in ((B, H, W), (B, H // 2, W // 2), (B, H // 2, W // 2))]
        out = dict(zip("yuv", planes))
        for ft, tag in ((torch.float32, "32"), (torch.float64, "64")):
            norm = tuple(torch.from_numpy(p.astype(np.float64)).to(ft).unsqueeze(1) / peak for p in planes)
            for mode in ("bilinear", "nearest"):
                out[f"rgb{tag}_{mode}"] = ref.ycbcr2rgb(to_444(norm, mode)).numpy()
        src = rng.random((B, 3, H, W), dtype=np.float32)
        out["src"] = src
        for ft, tag in ((torch.float32, "32"), (torch.float64, "64")):
            for n, p in zip("yuv", ref.yuv_444_to_420(ref.rgb2ycbcr(torch.from_numpy(src).to(ft)))):
                out[f"{n}{tag}"] = p.squeeze(1).numpy()
        # what the tests assert about the inputs
        for mode in ("bilinear", "nearest"):
            err = np.abs(out[f"rgb32_{mode}"].astype(np.float64) - out[f"rgb64_{mode}"]).max()
            assert err <= GATE, (case, mode, err)
        for n in "yuv":
            err = np.abs(out[f"{n}32"].astype(np.float64) - out[f"{n}64"]).max()
            assert err <= GATE, (case, n, err)
            share = (quantise(out[f"{n}32"].astype(np.float64), peak) != quantise(out[f"{n}64"], peak)).mean()
            assert share <= EXCUSED_SHARE, (case, n, share)
        inputs = ("y", "u", "v", "src")
        keep = list(range(B)) if H * W <= ALL_IMAGES_MAX_PIXELS else [B - 1]
        members[f"{case}/ref_images/0"] = np.array(keep, dtype=np.int64)
        for name, a in out.items():
            if name not in inputs and a.dtype == np.float32 and H * W > F32_MAX_PIXELS:
                continue
            for b in (range(B) if name in inputs else keep):
                members[f"{case}/{name}/{b}"] = np.ascontiguousarray(a[b])

    for old in glob.glob(STEM + "*.npz"):
        os.remove(old)
    part, size, index = {}, 0, 0

    def flush():
        nonlocal part, size, index
        if part:
            path = STEM + (".npz" if index == 0 else f".{index}.npz")
            np.savez_compressed(path, **part)
            assert os.path.getsize(path) < 1024 * 1024, path
            print(f"{path}: {len(part)} arrays, {os.path.getsize(path)} bytes")
            part, size, index = {}, 0, index + 1

    for k, a in members.items():
        if size + a.nbytes > PART_BYTES:
            flush()
        part[k] = a
        size += a.nbytes
    flush()


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
