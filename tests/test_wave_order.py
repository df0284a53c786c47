"""CPU: the wavefront symbol order (codec.wave_order, include/stem_ar_batch.h) as a pure function, the C ABI of its two entry points
(stem_ar_to_wave_order, stem_ar_decode_wave_batch) as the header, the ctypes reader and the library state it, the header flag of
bitstream.py, the `order` keyword's refusals, and the host coder popped in steps of varying length."""
import ctypes as C
import inspect
import io
import os
import re
import struct

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(1, 1), (1, 7), (5, 1), (4, 6), (7, 5), (3, 16), (68, 120)]


def _wave_range(t, H, W):
    """wave_range of csrc/ar_canon.h, restated: rows h0 .. h0 + np - 1 hold the positions of step t"""
    lo = t - (W - 1)
    lo = (lo + 2) // 3 if lo > 0 else 0
    hi = min(t // 3, H - 1)
    return lo, hi - lo + 1


@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_wave_order(H, W):
    from spatiotemporalentropymodel_amd.codec import wave_order
    order, sizes = wave_order(H, W)
    assert order.dtype == np.int64 and order.shape == (H * W,)
    assert sorted(order.tolist()) == list(range(H * W))                           # a permutation
    assert len(sizes) == W + 3 * (H - 1)                                          # the step count
    assert [int(s) for s in sizes] == [max(0, _wave_range(t, H, W)[1]) for t in range(len(sizes))]
    assert int(sizes.sum()) == H * W and int(sizes.max()) == min(H, (W + 2) // 3)
    # inside a step rows ascend from h0 with w = t - 3h; the rank of a position is the issue's closed form
    step_of = {}
    start = 0
    for t, n in enumerate(sizes.tolist()):
        h0 = _wave_range(t, H, W)[0]
        for p, r in enumerate(order[start:start + n].tolist()):
            h, w = divmod(r, W)
            assert (h, w) == (h0 + p, t - 3 * (h0 + p)), (t, p, h, w)
            step_of[(h, w)] = t
        start += n
    # every in-image neighbour among the 12 live taps of the 5x5 type-A mask lies in a strictly earlier step
    taps = [(dh, dw) for dh in (-2, -1) for dw in (-2, -1, 0, 1, 2)] + [(0, -2), (0, -1)]
    assert len(taps) == 12
    for (h, w), t in step_of.items():
        for dh, dw in taps:
            if 0 <= h + dh < H and 0 <= w + dw < W:
                assert step_of[(h + dh, w + dw)] < t, ((h, w), (dh, dw))


def test_wave_order_refuses_an_empty_latent():
    from spatiotemporalentropymodel_amd.codec import wave_order
    for bad in ((0, 4), (3, 0)):
        with pytest.raises(ValueError):
            wave_order(*bad)


def test_wave_entry_points_are_declared_and_bound():
    from spatiotemporalentropymodel_amd import _abi, _lib
    header = os.path.join(REPO, "include", "stem_ar_batch.h")
    text = open(header).read()
    protos = _abi.prototypes(header)
    hip = _abi.prototypes(os.path.join(REPO, "include", "stem_hip.h"))
    for name in ("stem_ar_to_wave_order", "stem_ar_decode_wave_batch"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m, f"{name} is not declared in include/stem_ar_batch.h"
        restype, argtypes = protos[name]
        assert restype is C.c_int and len(argtypes) == len([a for a in m.group(1).split(",") if a.strip()])
        assert name not in hip                                                    # one header per entry point
        assert getattr(C.CDLL(_lib.HIP_SO), name) is not None
        fn = getattr(_lib.hip(), name)                                            # bound with the header's prototype
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)
    assert _lib.declared_hip_batch_symbols() == sorted(protos)
    vp, i = C.c_void_p, C.c_int
    assert protos["stem_ar_to_wave_order"][1] == [vp, vp, vp, vp, i, i, i, i, vp]
    # stem_ar_decode_batch's arguments (the callback is a typedef of this header's own)
    assert list(protos["stem_ar_decode_wave_batch"][1]) == list(hip["stem_ar_decode_batch"][1])
    assert _lib.hip().stem_abi_version() == 5


def _decode_args(**kw):
    p = 4096                                         # never dereferenced: every call below fails its argument checks first
    handles = (C.c_void_p * 2)(p, p)
    ok = dict(w_ctx=p, ld_ctx=48, b_ctx=p, w0=p, ld0=24, b0=p, n0=16, w1=p, ld1=16, b1=p, n1=12, w2=p, ld2=12, b2=p, buf=p, G=2, H=4, W=6, M=4,
              pad=2, tp=p, hp=p, wctx=p, wh1=p, wh2=p, wgp=p, table=p, T=64, bound=0.11, slope=0.01, idx_host=p, sym_host=p, decode=p,
              decs=C.addressof(handles), cdfs=p, ncdf=64, cdf_stride=8, sizes=p, offsets=p)
    ok.update(kw)
    return ok, handles


def test_decode_wave_batch_argument_errors_name_the_function():
    """G = 0, NULL buf / hp / mailboxes / callback / handles, pad != 2, sizes and addresses off the grid: refused before anything
    touches a device"""
    from spatiotemporalentropymodel_amd import _lib
    h = _lib.hip()
    p = 4096

    def call(**kw):
        a, keep = _decode_args(**kw)
        return h.stem_ar_decode_wave_batch(*a.values(), None), h.stem_last_error()

    for bad in (dict(G=0), dict(G=-3), dict(buf=None), dict(hp=None), dict(idx_host=None), dict(sym_host=None), dict(decode=None), dict(decs=None),
                dict(wgp=None), dict(table=None), dict(pad=1), dict(pad=0), dict(pad=3), dict(H=0), dict(W=0), dict(M=6), dict(M=0), dict(n0=18),
                dict(n1=0), dict(ld0=26), dict(T=0), dict(buf=p + 4), dict(hp=p + 8), dict(tp=p + 4), dict(wh1=p + 4), dict(w2=p + 8),
                dict(idx_host=p + 2), dict(sym_host=p + 1)):
        rc, msg = call(**bad)
        assert rc != 0 and b"stem_ar_decode_wave_batch" in msg, (bad, rc, msg)
    assert b"got 0" in call(G=0)[1]
    handles = (C.c_void_p * 2)(p, None)                                           # an image without a decoder
    rc, msg = call(decs=C.addressof(handles))
    assert rc != 0 and b"stem_ar_decode_wave_batch" in msg and b"image 1" in msg


def test_to_wave_order_argument_errors_name_the_function():
    from spatiotemporalentropymodel_amd import _lib
    h = _lib.hip()
    p = 4096
    ok = dict(sym_raster=p, idx_raster=2 * p, sym_wave=3 * p, idx_wave=4 * p, G=2, H=4, W=6, M=4)
    for bad in (dict(sym_raster=None), dict(idx_raster=None), dict(sym_wave=None), dict(idx_wave=None), dict(G=0), dict(H=0), dict(W=-1), dict(M=0),
                dict(sym_wave=p), dict(idx_wave=2 * p)):
        rc = h.stem_ar_to_wave_order(*dict(ok, **bad).values(), None)
        msg = h.stem_last_error()
        assert rc != 0 and b"stem_ar_to_wave_order" in msg, (bad, rc, msg)


def test_header_flag_round_trip_and_raster_headers_unchanged():
    from spatiotemporalentropymodel_amd import bitstream as bs
    for name in bs.MODEL_NAMES:
        for quality in range(1, 9):
            raster = bs.get_header(name, "mse", quality)
            assert raster == (bs.model_ids[name], (bs.metric_ids["mse"] << 4) | (quality - 1 & 0x0F))      # the reference's two bytes
            assert raster == bs.get_header(name, "mse", quality, order="raster") and bs.stream_order(raster) == "raster"
            wave = bs.get_header(name, "mse", quality, order="wavefront")
            assert wave == (raster[0], raster[1] | 0x80) and all(0 <= b < 256 for b in wave)
            assert bs.stream_order(wave) == "wavefront"
            for header in (raster, wave):
                parsed = bs.parse_header(header)
                assert parsed == (name, "mse", quality) and len(parsed) == 3      # the same triple for both orders
                assert bs.stream_order(parsed) == bs.stream_order(header)
    with pytest.raises(ValueError):
        bs.get_header("mbt2018", "mse", 3, order="zigzag")


def test_frame_records_carry_the_order_and_raster_records_are_unchanged():
    from spatiotemporalentropymodel_amd import bitstream as bs
    strings = [[b"\x01\x02\x03\x04\x05\x06\x07\x08"], [b"abcdefgh1234"]]
    fd = io.BytesIO()
    bs.write_frame(fd, bs.get_header("mbt2018", "mse", 3), (120, 104), (2, 2), strings)
    want = struct.pack(">2B", 3, 2) + struct.pack(">2I", 120, 104) + struct.pack(">3I", 2, 2, 2)
    for s in strings:
        want += struct.pack(">I", len(s[0])) + s[0]
    assert fd.getvalue() == want                                                  # the layout of the reference tool, byte for byte
    fd = io.BytesIO()
    bs.write_sequence(fd, [(bs.get_header("mbt2018", "mse", 3, order), (120, 104), (2, 2), strings) for order in ("wavefront", "raster")])
    assert fd.getvalue()[4:6] == bytes([3, 0x82])
    fd.seek(0)
    frames = bs.read_sequence(fd)
    assert [bs.stream_order(f[0]) for f in frames] == ["wavefront", "raster"]
    for header, size, shape, got in frames:
        assert header == ("mbt2018", "mse", 3) and tuple(size) == (120, 104) and tuple(shape) == (2, 2) and got == strings


def test_unknown_orders_are_refused_before_any_work():
    from spatiotemporalentropymodel_amd import codec, evaluation
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res, SpatioTemporalPriorModelWithoutSPM
    from spatiotemporalentropymodel_amd.models.priors import JointAutoregressiveHierarchicalPriors
    stem, image, flat = SpatioTemporalPriorModel_Res(64, 96), JointAutoregressiveHierarchicalPriors(64, 96), SpatioTemporalPriorModelWithoutSPM(64, 96)
    calls = [lambda o: stem.compress(None, None, order=o), lambda o: stem.decompress([[b""], [b""]], (1, 1), None, order=o),
             lambda o: image.compress(None, order=o), lambda o: image.decompress([[b""], [b""]], (1, 1), order=o),
             lambda o: codec.stem_compress_each(stem, [], [], order=o), lambda o: codec.stem_decompress_each(stem, [], [], [], order=o),
             lambda o: codec.iframe_compress_each(image, [], order=o), lambda o: codec.iframe_decompress_each(image, [], [], order=o),
             lambda o: codec._encode_latents(stem, None, None, None, order=o), lambda o: codec._decode_latents(stem, [], None, None, order=o),
             lambda o: evaluation.inference_iframe(image, None, order=o), lambda o: evaluation.inference_pframe(image, stem, None, None, order=o),
             lambda o: evaluation.eval_gop(image, stem, [], order=o), lambda o: evaluation.eval_sequence(image, stem, [], order=o)]
    for call in calls:
        with pytest.raises(ValueError, match="zigzag"):
            call("zigzag")
    # no spatial prior: no raster loop, nothing to reorder
    for call in (lambda: flat.compress(None, None, order="wavefront"), lambda: flat.decompress([[b""], [b""]], (1, 1), None, order="wavefront"),
                 lambda: codec.stem_compress_each(flat, [], [], order="wavefront"), lambda: codec.stem_decompress_each(flat, [], [], [], order="wavefront")):
        with pytest.raises(ValueError, match="spatial prior"):
            call()


def test_the_order_keyword_defaults_to_raster_everywhere():
    from spatiotemporalentropymodel_amd import bitstream, codec, evaluation
    from spatiotemporalentropymodel_amd.models import (SpatioTemporalPriorModel, SpatioTemporalPriorModel_Res, SpatioTemporalPriorModelWithoutSPM,
                                                       SpatioTemporalPriorModelWithoutSPMTPM, SpatioTemporalPriorModelWithoutTPM)
    from spatiotemporalentropymodel_amd.models.priors import JointAutoregressiveHierarchicalPriors
    fns = [codec.stem_compress, codec.stem_decompress, codec.stem_compress_each, codec.stem_decompress_each, codec.iframe_compress,
           codec.iframe_decompress, codec.iframe_compress_each, codec.iframe_decompress_each, codec._encode_latents, codec._decode_latents,
           evaluation.inference_iframe, evaluation.inference_pframe, evaluation.eval_gop, evaluation.eval_sequence, bitstream.get_header]
    for cls in (SpatioTemporalPriorModel, SpatioTemporalPriorModel_Res, SpatioTemporalPriorModelWithoutSPM, SpatioTemporalPriorModelWithoutSPMTPM,
                SpatioTemporalPriorModelWithoutTPM, JointAutoregressiveHierarchicalPriors):
        fns += [cls.compress, cls.decompress]
    for fn in fns:
        assert inspect.signature(fn).parameters["order"].default == "raster", fn
    assert "order" not in inspect.signature(codec.decode_route).parameters


def test_host_coder_pops_one_string_in_steps_of_varying_length():
    """symbols and indexes with escape values, encoded by ONE encode_with_indexes call and popped by one decode call per wavefront step
    (n = np(t) * M symbols, n = 0 for the empty steps of a one-column latent): they come back exactly, and the string is used up"""
    from spatiotemporalentropymodel_amd.codec import wave_order
    from spatiotemporalentropymodel_amd.entropy_models import BufferedRansEncoder, GaussianConditional, RansDecoder
    gc = GaussianConditional(None)
    gc.update_scale_table([0.11, 0.3, 1.0, 3.0, 9.0], force=True)
    tables = gc.host_tables()
    rng = np.random.default_rng(7)
    for (H, W), M in (((7, 5), 4), ((5, 1), 8), ((3, 16), 4)):
        sizes = wave_order(H, W)[1] * M
        n = int(sizes.sum())
        idx = rng.integers(0, len(tables.sizes), n).astype(np.int32)
        sym = np.rint(rng.normal(0.0, 2.0, n)).astype(np.int32)
        sym[::17] = rng.integers(-3000, 3000, len(sym[::17]))                     # far outside every table row
        lo, hi = tables.offsets[idx], tables.offsets[idx] + tables.sizes[idx] - 2
        assert ((sym < lo) | (sym >= hi)).sum() >= 3 and ((sym >= lo) & (sym < hi)).sum() >= 3      # escapes and plain symbols
        enc = BufferedRansEncoder()
        enc.encode_with_indexes(sym, idx, tables)
        string = enc.flush()
        dec = RansDecoder()
        dec.set_stream(string)
        got, start = [], 0
        for s in sizes.tolist():
            got.append(dec.decode_stream_np(idx[start:start + s], tables))
            assert got[-1].shape == (s,)
            start += s
        assert 0 in sizes.tolist() or W >= 3
        assert np.array_equal(np.concatenate(got), sym)
        assert np.array_equal(RansDecoder().decode_with_indexes_np(string, idx, tables), sym)
        with pytest.raises(RuntimeError, match="exhausted"):                      # every word of the string has been read
            dec.decode_stream_np(idx[:1], tables)
