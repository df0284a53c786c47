"""GPU: the pixel-domain sequence codec (spatiotemporalentropymodel_amd/video_pixel.py) against evaluation.eval_gop_pixel, whose strings and
reconstructions the existing suite pins to the reference: every record holds its strings, the decoder -- also a fresh process that has
only the file and two checkpoints -- rebuilds its frames.  Equality everywhere, no tolerance."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pixel_eval_fixture as fx
import roi_map_ref
from conftest import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOP = 3
LEVEL = 0.25


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def pairs(golden):
    """name -> (model_i, model_p), on the closed-form weights of tests/pixel_eval_fixture.py, built once"""
    from spatiotemporalentropymodel_amd.models import stem_roi_wo_gsc
    groi, gbase = golden("pixel_eval_roi.npz"), golden("pixel_eval_baseline.npz")
    roi_i, roi_p = fx.roi_chain(DEV, groi)
    return {"roi": (roi_i, roi_p), "wo_gsc": (roi_i, fx.build(stem_roi_wo_gsc, "roi_wo", fx.ROI_CONV_SCALE, DEV)), "baseline": fx.baseline_chain(DEV, gbase)}


@pytest.fixture(scope="module")
def frames5():
    """five 122 x 126 frames (odd offsets 3, 1 in 128 x 128): I P P I P under gop 3"""
    from spatiotemporalentropymodel_amd.weights import smooth_frames
    return [f[0, :, 3:125, 1:127].contiguous().to(DEV) for f in smooth_frames("videopixel", 1, 5, 128)]


@pytest.fixture(scope="module")
def frames3():
    return [f.to(DEV) for f in fx.frames3()]


def _qmap(h, w, tag="q"):
    from spatiotemporalentropymodel_amd.weights import closed_form_input
    return closed_form_input(f"videopixel:{tag}", (1, 1, h, w), 0.0, 1.0)


def _boxes(index, h, w):
    return [(10 + 7 * index, 20, 70 + 7 * index, 90, 0.875, 5), (-8, 60 - 3 * index, 40, h + 9, 0.5, 2), (w - 30, 4, w - 6, 30, 1.0)]


def _maps_for(form, n, h, w):
    """-> (encode_sequence's keywords, eval_gop_pixel's qmaps) of one form of quality information"""
    if form is None:
        return {}, None
    if form == "tensor":
        q = _qmap(h, w)
        return {"qmaps": q}, q
    if form == "iterable":
        qs = [_qmap(h, w, f"q{k}") for k in range(n)]
        return {"qmaps": iter(qs)}, iter(qs)
    rois = [_boxes(k, h, w) for k in range(n)]
    return {"rois": rois if form == "rois" else (lambda k: rois[k]), "level": LEVEL}, \
        [torch.from_numpy(roi_map_ref.roi_map(b, (h, w), LEVEL)) for b in rois]


@pytest.fixture(scope="module")
def reference(pairs, frames5, frames3):
    """(pair, frames, form) -> eval_gop_pixel's result, computed once and left alone"""
    from spatiotemporalentropymodel_amd import evaluation
    cache = {}

    def get(pair, which, form, all_intra=False):
        key = (pair, which, form, all_intra)
        if key not in cache:
            frames = frames5 if which == 5 else frames3
            h, w = frames[0].shape[-2:]
            cache[key] = evaluation.eval_gop_pixel(*pairs[pair], frames, qmaps=_maps_for(form, len(frames), h, w)[1], gop=GOP, all_intra=all_intra,
                                                   with_msssim=False, roi_weight=False)
        return cache[key]

    return get


def _encode(pairs, pair, frames, form, **kw):
    from spatiotemporalentropymodel_amd import video_pixel
    h, w = frames[0].shape[-2:]
    buf = io.BytesIO()
    res = video_pixel.encode_sequence(*pairs[pair], frames, buf, gop=GOP, **_maps_for(form, len(frames), h, w)[0], **kw)
    return buf.getvalue(), res


def _records(data):
    from spatiotemporalentropymodel_amd import video_pixel
    hdr = video_pixel.FileHeader.unpack(data)
    ranges = video_pixel.record_ranges(data, hdr.frames, video_pixel.HEADER_BYTES)
    return hdr, [video_pixel.read_record(data, ranges[k], hdr, k, t) + (data[ranges[k][0]],) for k, t in enumerate(hdr.types())]


# ----------------------------------------------------------------------------- 1. the encoder's own reconstruction
@pytest.mark.parametrize("name", ["stem_baseline", "stem_baselinev2", "stem_roi", "stem_roi_wo_gsc", "stem_roi_i"])
def test_compress_returns_what_decompress_returns(name, pairs, frames5):
    from spatiotemporalentropymodel_amd import bitstream, models
    have = {"stem_roi_i": pairs["roi"][0], "stem_roi": pairs["roi"][1], "stem_roi_wo_gsc": pairs["wo_gsc"][1], "stem_baseline": pairs["baseline"][1]}
    m = have.get(name) or fx.build(getattr(models, name), "base_v2", fx.ROI_CONV_SCALE, DEV)
    with torch.no_grad():
        x, xc = (bitstream.pad(f.unsqueeze(0), 64) for f in frames5[:2])
        q = bitstream.pad(_qmap(122, 126).to(DEV), 64)
        args = [x] + ([xc] if m.TEMPORAL else []) + ([q] if m.QMAP else [])
        plain = m.compress(*args)
        assert sorted(plain) == ["shape", "strings"]                                   # without the keyword: today's dictionary
        enc = m.compress(*args, return_x_hat=True)
        assert sorted(enc) == ["shape", "strings", "x_hat"] and enc["strings"] == plain["strings"] and tuple(enc["shape"]) == tuple(plain["shape"])
        dec = m.decompress(enc["strings"], enc["shape"], *([xc] if m.TEMPORAL else []))
    assert enc["x_hat"].shape == dec["x_hat"].shape == x.shape and enc["x_hat"].is_contiguous()
    assert torch.equal(_bits(enc["x_hat"]), _bits(dec["x_hat"]))
    assert float(enc["x_hat"].std()) > 0


# ----------------------------------------------------------------------------- 2. the records
@pytest.mark.parametrize("pair,form", [("roi", "tensor"), ("roi", "iterable"), ("roi", "rois"), ("wo_gsc", "tensor"), ("baseline", None)])
def test_records_hold_eval_gop_pixels_strings_and_no_decoder_runs(pair, form, pairs, frames5, reference, monkeypatch):
    from spatiotemporalentropymodel_amd import bitstream, video_pixel
    ref = reference(pair, 5, form)

    def no_decoder(*a, **k):
        raise AssertionError("the encoder called decompress")

    for m in pairs[pair]:
        monkeypatch.setattr(m, "decompress", no_decoder)
    data, res = _encode(pairs, pair, frames5, form)
    hdr, recs = _records(data)
    assert hdr.types() == [f["type"] for f in ref["frames"]] == ["I", "P", "P", "I", "P"] == [f["type"] for f in res["frames"]]
    assert (hdr.height, hdr.width, hdr.bit_depth, hdr.frames, hdr.gop, hdr.all_intra, hdr.quality) == (122, 126, 8, 5, GOP, 0, 4)
    for k, ((shape, strings, first), want) in enumerate(zip(recs, ref["frames"])):
        assert strings == want["strings"], f"{pair}/{form}: the strings of frame {k} differ from eval_gop_pixel's"
        assert tuple(shape) == tuple(want["shape"])
        assert first == hdr.record_byte(want["type"]) and res["frames"][k]["bpp"] == want["bpp"]
    assert res["bytes"] == len(data) == video_pixel.HEADER_BYTES + sum(f["bytes"] for f in res["frames"])
    assert res["bpp_ave"] == sum(f["bpp"] for f in ref["frames"]) / 5
    if pair == "baseline":                                                              # a zoo I record is the reference tool's record
        want = io.BytesIO()
        bitstream.write_frame(want, bitstream.get_header("mbt2018-mean", "mse", 4), (122, 126), ref["frames"][0]["shape"], ref["frames"][0]["strings"])
        assert data[42:42 + res["frames"][0]["bytes"]] == want.getvalue()
    if form == "rois":                                                                  # a callable gives the same file
        assert _encode(pairs, pair, frames5, "rois callable")[0] == data
        # and the rectangles changed the rate: the records are not those of the flat background
        flat, _ = _encode(pairs, pair, frames5[:1], None, rois=[[]], level=LEVEL)
        assert _records(flat)[1][0][1] != recs[0][1]


# ----------------------------------------------------------------------------- 3. the decoder
@pytest.fixture(scope="module")
def coded(pairs, frames5):
    """pair -> the file of frames5 (bytes), written once"""
    return {"roi": _encode(pairs, "roi", frames5, "rois")[0], "wo_gsc": _encode(pairs, "wo_gsc", frames5, "tensor")[0],
            "baseline": _encode(pairs, "baseline", frames5, None)[0]}


def _planes_file(x_hats, bits):
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd.video import _planes_bytes
    return b"".join(_planes_bytes(F.rgb_window_to_yuv420(x.contiguous(), x.shape[-2:], bits)) for x in x_hats)


@pytest.mark.parametrize("pair,form", [("roi", "rois"), ("wo_gsc", "tensor"), ("baseline", None)])
def test_the_decoder_rebuilds_eval_gop_pixels_frames(pair, form, pairs, coded, reference):
    from spatiotemporalentropymodel_amd import video_pixel
    ref = reference(pair, 5, form)
    sink = io.BytesIO()
    got = video_pixel.decode_sequence(*pairs[pair], coded[pair], write_to=sink)
    assert len(got) == 5
    for k, (a, want) in enumerate(zip(got, ref["frames"])):
        assert tuple(a.shape) == (1, 3, 122, 126) and a.is_contiguous()
        assert torch.equal(_bits(a), _bits(want["x_hat"])), f"{pair}: frame {k} differs from eval_gop_pixel's x_hat"
    assert sink.getvalue() == _planes_file([f["x_hat"] for f in ref["frames"]], 8)
    # without a file, and without the tensors
    again = video_pixel.decode_sequence(*pairs[pair], io.BytesIO(coded[pair]))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, got))
    sink2 = io.BytesIO()
    assert video_pixel.decode_sequence(*pairs[pair], coded[pair], write_to=sink2, return_frames=False) == [] and sink2.getvalue() == sink.getvalue()
    # frames=(3, 5): a slice of the full decode; (1, 3) starts inside a GOP
    for start, stop in ((3, 5), (1, 3), (4, 5)):
        sink3 = io.BytesIO()
        part = video_pixel.decode_sequence(*pairs[pair], coded[pair], write_to=sink3, frames=(start, stop))
        assert len(part) == stop - start and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(part, got[start:stop]))
        per = len(sink.getvalue()) // 5
        assert sink3.getvalue() == sink.getvalue()[start * per:stop * per]


def test_a_forward_pass_between_encode_and_decode_changes_nothing(pairs, frames5, coded, reference):
    from spatiotemporalentropymodel_amd import bitstream, video_pixel
    model_i, model_p = pairs["roi"]
    with torch.no_grad():
        x, xc = (bitstream.pad(f.unsqueeze(0), 64) for f in frames5[:2])
        q = bitstream.pad(_qmap(122, 126).to(DEV), 64)
        model_i(x, q), model_p(x, xc, q)
    got = video_pixel.decode_sequence(model_i, model_p, coded["roi"])
    for a, want in zip(got, reference("roi", 5, "rois")["frames"]):
        assert torch.equal(_bits(a), _bits(want["x_hat"]))
    assert _encode(pairs, "roi", frames5, "rois")[0] == coded["roi"]


def test_all_intra_and_the_fixtures_frames(pairs, frames3, reference):
    from spatiotemporalentropymodel_amd import video_pixel
    ref = reference("roi", 3, "tensor", True)
    data, res = _encode(pairs, "roi", frames3, "tensor", all_intra=True)
    hdr, recs = _records(data)
    assert hdr.types() == ["I"] * 3 and hdr.all_intra == 1 and hdr.p_kind == video_pixel.NO_P and (hdr.height, hdr.width) == fx.SIZE
    assert [r[1] for r in recs] == [f["strings"] for f in ref["frames"]]
    got = video_pixel.decode_sequence(pairs["roi"][0], None, data)
    assert all(torch.equal(_bits(a), _bits(f["x_hat"])) for a, f in zip(got, ref["frames"]))
    # the same frames as one GOP: I P P
    ref = reference("roi", 3, "tensor")
    data, _ = _encode(pairs, "roi", frames3, "tensor")
    assert [r[1] for r in _records(data)[1]] == [f["strings"] for f in ref["frames"]]
    sink = io.BytesIO()
    got = video_pixel.decode_sequence(*pairs["roi"], data, write_to=sink)
    assert all(torch.equal(_bits(a), _bits(f["x_hat"])) for a, f in zip(got, ref["frames"]))
    assert sink.getvalue() == _planes_file([f["x_hat"] for f in ref["frames"]], 8)


def test_a_ten_bit_sequence_file_in_and_out(pairs, frames3, tmp_path):
    """the input is a data.YUVSequence (integer planes through the ingest kernel), the output a 10-bit file"""
    from spatiotemporalentropymodel_amd import data, evaluation, video_pixel
    src = tmp_path / "in10.yuv"
    for k, f in enumerate(frames3):
        data.write_yuv420(str(src), f, bit_depth=10, append=k > 0)
    h, w = fx.SIZE
    seq = data.YUVSequence(str(src), w, h, 10, device=DEV)
    q = _qmap(h, w)
    ref = evaluation.eval_gop_pixel(*pairs["roi"], seq, qmaps=q, gop=GOP, with_msssim=False, roi_weight=False)
    coded_path, out = tmp_path / "ten.stpx", tmp_path / "out10.yuv"
    video_pixel.encode_sequence(*pairs["roi"], seq, str(coded_path), qmaps=q, gop=GOP)
    blob = coded_path.read_bytes()
    hdr, recs = _records(blob)
    assert hdr.bit_depth == 10 and [r[1] for r in recs] == [f["strings"] for f in ref["frames"]]
    got = video_pixel.decode_sequence(*pairs["roi"], str(coded_path), write_to=str(out))
    assert all(torch.equal(_bits(a), _bits(f["x_hat"])) for a, f in zip(got, ref["frames"]))
    assert out.read_bytes() == _planes_file([f["x_hat"] for f in ref["frames"]], 10) and len(out.read_bytes()) == 3 * h * w * 3
    back = data.YUVSequence(str(out), w, h, 10, device=DEV)
    assert len(back) == 3


def test_a_fresh_process_decodes_the_file_alone(pairs, coded, reference, tmp_path):
    """the command line in a child process that has the file and two checkpoints, nothing else of this process"""
    model_i, model_p = pairs["roi"]
    ick, pck, src, out = tmp_path / "i.pt", tmp_path / "p.pt", tmp_path / "in.stpx", tmp_path / "child.yuv"
    torch.save(model_i.state_dict(), ick)
    torch.save(model_p.state_dict(), pck)
    src.write_bytes(coded["roi"])
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "spatiotemporalentropymodel_amd.video_pixel", "decode", "--model-i", "stem_roi_i", "--model-i-checkpoint",
                        str(ick), "--model-p", "stem_roi", "--model-p-checkpoint", str(pck), "--input", str(src), "--output", str(out)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert out.read_bytes() == _planes_file([f["x_hat"] for f in reference("roi", 5, "rois")["frames"]], 8)


def test_refusals(pairs, frames5, coded):
    from spatiotemporalentropymodel_amd import video_pixel
    from spatiotemporalentropymodel_amd.models import stem_roi
    model_i, model_p = pairs["roi"]
    other = fx.build(stem_roi, "roi_p_other", fx.ROI_CONV_SCALE, DEV)
    with pytest.raises(ValueError, match="P-frame model's weights"):
        video_pixel.decode_sequence(model_i, other, coded["roi"])
    with pytest.raises(ValueError, match="P-frame model"):
        video_pixel.decode_sequence(model_p, model_i, coded["roi"])
    with pytest.raises(ValueError, match="coded with stem_roi,"):
        video_pixel.decode_sequence(model_i, pairs["wo_gsc"][1], coded["roi"])
    with pytest.raises(ValueError, match="coded with mbt2018-mean"):
        video_pixel.decode_sequence(model_i, model_p, coded["baseline"])
    with pytest.raises(ValueError, match="truncated"):
        video_pixel.decode_sequence(model_i, model_p, coded["roi"][:-1])
    out = io.BytesIO()
    with pytest.raises(ValueError, match="takes a quality map"):
        video_pixel.encode_sequence(model_i, model_p, frames5, out, gop=GOP)
    with pytest.raises(ValueError, match="takes a quality map"):
        video_pixel.encode_sequence(pairs["baseline"][0], model_p, frames5, out, gop=GOP)
    with pytest.raises(ValueError, match="none of the coding models"):
        video_pixel.encode_sequence(*pairs["baseline"], frames5, out, gop=GOP, qmaps=_qmap(122, 126))
    assert out.getvalue() == b""
    with pytest.raises(ValueError, match="frame 1 has none"):                          # a callable that stops giving maps
        video_pixel.encode_sequence(model_i, model_p, frames5, io.BytesIO(), gop=GOP, qmaps=lambda k, h, w: _qmap(h, w) if k == 0 else None)
    with pytest.raises(ValueError, match="ran out"):
        video_pixel.encode_sequence(model_i, model_p, frames5, io.BytesIO(), gop=GOP, rois=[[]] * 2)
    with pytest.raises(ValueError, match="roi_map_padded"):
        video_pixel.encode_sequence(model_i, model_p, frames5, io.BytesIO(), gop=GOP, rois=lambda k: [(5, 5, 5, 9, 0.5)])
