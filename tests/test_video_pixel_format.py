"""CPU: the file format of the pixel-domain sequence codec (spatiotemporalentropymodel_amd/video_pixel.py) -- header, record bytes, the
helpers it shares with video.py, the command line's parsing -- and every refusal that needs no device."""
import io
import struct

import pytest
import torch

from spatiotemporalentropymodel_amd import bitstream, video, video_pixel


@pytest.fixture(scope="module")
def models():
    """small CPU models: nothing here runs a kernel"""
    from spatiotemporalentropymodel_amd.models import stem_baseline, stem_roi, stem_roi_i, stem_roi_wo_gsc
    from spatiotemporalentropymodel_amd.models.priors import FactorizedPrior, MeanScaleHyperprior
    torch.manual_seed(0)
    out = {"roi_i": stem_roi_i(8, 16), "roi_i_other": stem_roi_i(8, 16), "roi_i_wide": stem_roi_i(8, 24), "roi": stem_roi(8, 16),
           "wo_gsc": stem_roi_wo_gsc(8, 16), "base": stem_baseline(8, 16), "mean": MeanScaleHyperprior(8, 16), "factorized": FactorizedPrior(8, 16)}
    for m in out.values():
        m.eval().update(force=True)
    return out


def _strings(k):
    return [[bytes([k, 1, 2, 3] * (k + 1))], [bytes([9, k])]]


def _file(models, n=5, gop=3, all_intra=False, i="roi_i", p="roi"):
    """a well-formed file with made-up strings -> (bytes, header, the records' bytes)"""
    hdr = video_pixel._header_for(models[i], models[p] if p else None, 120, 104, 8, n, gop, all_intra, 4)
    recs = [video_pixel.record_bytes(hdr.record_byte(t), 4, (120, 104), (2, 2), _strings(k)) for k, t in enumerate(hdr.types())]
    return hdr.pack() + b"".join(recs), hdr, recs


def test_the_header_round_trips(models):
    data, hdr, _ = _file(models)
    assert len(hdr.pack()) == video_pixel.HEADER_BYTES == video.HEADER_BYTES == 42 and data[:4] == b"STPX" and data[4] == video_pixel.VERSION == 1
    assert video_pixel._HEADER.format == video._HEADER.format
    back = video_pixel.FileHeader.unpack(data)
    assert back == hdr and back.pack() == hdr.pack()
    assert (back.width, back.height, back.bit_depth, back.frames, back.gop, back.all_intra, back.quality) == (104, 120, 8, 5, 3, 0, 4)
    assert back.i_kind == 64 and back.i_name == "stem_roi_i" and (back.i_a, back.i_b) == (8, 16)
    assert video_pixel.PIXEL_P_CLASSES == ("stem_baseline", "stem_baselinev2", "stem_roi", "stem_roi_wo_gsc")
    assert video_pixel.PIXEL_P_CLASSES[back.p_kind] == "stem_roi" and (back.p_a, back.p_b) == (8, 16)
    assert back.i_crc == video.fingerprint(models["roi_i"]) and back.p_crc == video.fingerprint(models["roi"])
    assert back.types() == ["I", "P", "P", "I", "P"]
    zoo = video_pixel._header_for(models["mean"], models["base"], 64, 64, 10, 3, 12, False, 4)
    assert zoo.i_kind == bitstream.model_ids["mbt2018-mean"] and zoo.i_name == "mbt2018-mean" and (zoo.i_a, zoo.i_b) == (8, 16) and zoo.p_kind == 0
    intra = video_pixel._header_for(models["roi_i"], None, 64, 64, 10, 3, 12, True, 4)
    assert intra.p_kind == video_pixel.NO_P == 255 and video_pixel.FileHeader.unpack(intra.pack()) == intra and intra.types() == ["I"] * 3
    unused = video_pixel._header_for(models["roi_i"], models["roi"], 64, 64, 8, 3, 12, True, 4)                    # all intra: the P model is not named
    assert unused.p_kind == 255 and unused.p_crc == 0


def test_the_header_refuses(models):
    data, hdr, _ = _file(models)
    with pytest.raises(ValueError, match="magic"):
        video_pixel.FileHeader.unpack(b"XXXX" + data[4:])
    with pytest.raises(ValueError, match="version"):
        video_pixel.FileHeader.unpack(data[:4] + bytes([2]) + data[5:])
    for cut in (0, 3, 4, 5, 41):
        with pytest.raises(ValueError, match="truncated"):
            video_pixel.FileHeader.unpack(data[:cut])
    # a file of the latent-domain codec: the other module is named; and video.py refuses this module's files
    from spatiotemporalentropymodel_amd.models import SpatioTemporalPriorModel_Res
    stmv = video._header_for(models["mean"], SpatioTemporalPriorModel_Res(8, 16), 120, 104, 8, 2, 2, False, 4).pack()
    with pytest.raises(ValueError, match=r"spatiotemporalentropymodel_amd\.video\b"):
        video_pixel.FileHeader.unpack(stmv + b"\0" * 64)
    with pytest.raises(ValueError, match="STMV"):
        video_pixel.decode_sequence(models["roi_i"], models["roi"], stmv + b"\0" * 64)
    with pytest.raises(ValueError):
        video.FileHeader.unpack(data)

    def repack(**kw):
        fields = dict(zip(video_pixel._FIELDS, hdr.astuple()), **kw)
        return video_pixel._HEADER.pack(b"STPX", 1, *(fields[k] for k in video_pixel._FIELDS))

    for kw in (dict(width=103), dict(height=121), dict(width=0), dict(bit_depth=9), dict(frames=0), dict(gop=0), dict(all_intra=2), dict(i_kind=6),
               dict(i_kind=63), dict(i_kind=65), dict(p_kind=4), dict(p_kind=254), dict(p_kind=255)):
        with pytest.raises(ValueError):
            video_pixel.FileHeader.unpack(repack(**kw))
    assert video_pixel.FileHeader.unpack(repack(p_kind=255, all_intra=1)).types() == ["I"] * 5
    with pytest.raises(ValueError, match="even sides"):
        video_pixel._header_for(models["roi_i"], models["roi"], 121, 104, 8, 5, 3, False, 4).pack()


def test_a_record_is_write_frames_bytes_under_the_first_byte_rule(models):
    strings = _strings(3)
    _, hdr, _ = _file(models)
    assert hdr.record_byte("I") == 64 and hdr.record_byte("P") == 128 + 2
    _, zoo, _ = _file(models, i="mean", p="base")
    assert zoo.record_byte("I") == bitstream.model_ids["mbt2018-mean"] and zoo.record_byte("P") == 128
    for quality in (1, 4, 8, 16):
        # for a zoo I-frame model an I record is byte for byte the reference tool's
        want = io.BytesIO()
        bitstream.write_frame(want, bitstream.get_header("mbt2018-mean", "mse", quality), (120, 104), (2, 2), strings)
        rec = video_pixel.record_bytes(zoo.record_byte("I"), quality, (120, 104), (2, 2), strings)
        assert rec == want.getvalue() and rec[1] == (quality - 1) & 0x0F
    rec = video_pixel.record_bytes(hdr.record_byte("P"), 4, (120, 104), (5, 7), strings)
    assert rec[:2] == bytes([130, 3]) and struct.unpack_from(">IIIII", rec, 2) == (120, 104, 5, 7, 2)
    assert video.record_ranges(rec, 1, 0) == [(0, len(rec))]
    assert video_pixel.read_record(rec, (0, len(rec)), hdr, 0, "P") == ((5, 7), strings)
    with pytest.raises(ValueError, match="record 0"):
        video_pixel.read_record(rec, (0, len(rec)), hdr, 0, "I")


def test_the_shared_helpers_are_videos(models):
    for name in ("_Source", "_open", "frame_types", "decode_steps", "record_ranges", "fingerprint", "_planes_bytes"):
        assert getattr(video_pixel, name) is getattr(video, name), name
    types = video_pixel.frame_types(5, 3)
    assert types == ["I", "P", "P", "I", "P"] and video_pixel.frame_types(5, 3, True) == ["I"] * 5
    assert video_pixel.decode_steps(types, 1) == [[(k, t, k // 3)] for k, t in enumerate(types)]
    assert video_pixel.decode_steps(types, 1, 3, 5) == [[(3, "I", 1)], [(4, "P", 1)]]
    assert video_pixel.decode_steps(types, 1, 1, 2) == [[(0, "I", 0)], [(1, "P", 0)]]
    data, hdr, recs = _file(models)
    ranges = video_pixel.record_ranges(data, hdr.frames, video_pixel.HEADER_BYTES)
    assert [b - a for a, b in ranges] == [len(r) for r in recs] and ranges[0][0] == 42 and ranges[-1][1] == len(data)


def test_the_decoder_refuses_before_any_device_work(models):
    """every refusal below is raised from the bytes and the models' state alone: the models are host models, and nothing is decoded"""
    data, hdr, recs = _file(models)
    i, p = models["roi_i"], models["roi"]
    # truncation at every structural boundary, and inside every field of the first record
    starts = [42 + sum(len(r) for r in recs[:k]) for k in range(len(recs))]
    cuts = set(range(0, 42, 7)) | {41}
    for s, r in zip(starts, recs):
        cuts |= {s, s + 1, s + 2, s + 10, s + 21, s + 22, s + 25, s + 26, s + len(r) - 1}
    for cut in sorted(cuts):
        with pytest.raises(ValueError, match="truncated"):
            video_pixel.decode_sequence(i, p, data[:cut])
    with pytest.raises(ValueError, match="behind the last"):
        video_pixel.decode_sequence(i, p, data + b"\0")
    # a record against the header: first byte (an I record where a P record belongs and the reverse, another kind), frame size
    for first in (130, 0, 65):
        with pytest.raises(ValueError, match="record 0 starts with byte"):
            video_pixel.decode_sequence(i, p, data[:42] + bytes([first]) + data[43:])
    with pytest.raises(ValueError, match="record 0 holds a frame"):
        video_pixel.decode_sequence(i, p, data[:44] + struct.pack(">I", 122) + data[48:])
    # the models: class, widths, fingerprint, presence
    with pytest.raises(ValueError, match="coded with stem_roi,"):
        video_pixel.decode_sequence(i, models["wo_gsc"], data)
    with pytest.raises(ValueError, match="coded with stem_roi_i"):
        video_pixel.decode_sequence(models["mean"], p, data)
    with pytest.raises(ValueError, match="widths"):
        video_pixel.decode_sequence(models["roi_i_wide"], p, data)
    with pytest.raises(ValueError, match="I-frame model's weights"):
        video_pixel.decode_sequence(models["roi_i_other"], p, data)
    with pytest.raises(ValueError, match="P-frame model is needed"):
        video_pixel.decode_sequence(i, None, data)
    with pytest.raises(ValueError, match="P-frame model"):                                 # swapped
        video_pixel.decode_sequence(p, i, data)
    with pytest.raises(ValueError, match="none of the pixel-domain P-frame classes"):
        video_pixel.decode_sequence(i, models["roi_i_other"], data)
    with pytest.raises(ValueError, match=r"video\.encode_sequence"):                        # a zoo model without getX
        video_pixel._header_for(models["factorized"], None, 64, 64, 8, 3, 12, True, 4)
    with pytest.raises(ValueError, match="no range"):
        video_pixel.decode_sequence(i, p, data, frames=(3, 9))


def test_the_encoder_refuses_before_any_device_work(models):
    frames = [torch.zeros(3, 8, 12)] * 3
    i, p, out = models["roi_i"], models["roi"], io.BytesIO()
    q = torch.zeros(8, 12)
    with pytest.raises(ValueError, match="mutually exclusive"):
        video_pixel.encode_sequence(i, p, frames, out, qmaps=q, rois=[[]] * 3)
    with pytest.raises(ValueError, match="takes a quality map"):
        video_pixel.encode_sequence(i, p, frames, out)
    with pytest.raises(ValueError, match="takes a quality map"):
        video_pixel.encode_sequence(models["mean"], p, frames, out)
    with pytest.raises(ValueError, match="none of the coding models takes one"):
        video_pixel.encode_sequence(models["mean"], models["base"], frames, out, qmaps=q)
    with pytest.raises(ValueError, match="none of the coding models takes one"):            # all intra: the P model codes nothing
        video_pixel.encode_sequence(models["mean"], p, frames, out, rois=[[]] * 3, all_intra=True)
    with pytest.raises(ValueError, match="P-frame model is needed"):
        video_pixel.encode_sequence(i, None, frames, out, qmaps=q)
    with pytest.raises(ValueError, match="even sides"):
        video_pixel.encode_sequence(i, p, [torch.zeros(3, 7, 12)], out, qmaps=q)
    with pytest.raises(ValueError, match=r"video\.encode_sequence"):
        video_pixel.encode_sequence(models["factorized"], models["base"], frames, out)
    with pytest.raises(TypeError):                                                          # the options are keyword-only
        video_pixel.encode_sequence(i, p, frames, out, q)
    assert out.getvalue() == b""


def test_roi_arguments_parse():
    assert video_pixel.parse_roi("1,2,30,40,0.75") == (1, 2, 30, 40, 0.75)
    assert video_pixel.parse_roi("-4,0,30,40,1,3") == (-4, 0, 30, 40, 1.0, 3)
    for bad in ("1,2,3,4", "1,2,3,4,0.5,1,2", "a,2,3,4,0.5", "1,2,3,4,x", "1,2,3,4,0.5,1.5", "1.5,2,3,4,0.5", ""):
        with pytest.raises(ValueError, match="--roi is"):
            video_pixel.parse_roi(bad)
    text = """# frame x0 y0 x1 y1 value [feather]
    0 1 2 30 40 0.75
    0 5 6 7 8 1 2      # a second box of frame 0

    3 -4 0 30 40 0.5 3
    """
    assert video_pixel.parse_roi_file(text.splitlines()) == {0: [(1, 2, 30, 40, 0.75), (5, 6, 7, 8, 1.0, 2)], 3: [(-4, 0, 30, 40, 0.5, 3)]}
    assert video_pixel.parse_roi_file(["# nothing", "   "]) == {}
    for bad in ("0 1 2 3 4", "0 1 2 3 4 0.5 1 9", "x 1 2 3 4 0.5", "-1 1 2 3 4 0.5", "0 1 2 3 4 0.5 1.5"):
        with pytest.raises(ValueError, match="--roi-file line 2"):
            video_pixel.parse_roi_file(["# ok", bad])
    args = video_pixel._parser().parse_args(["encode", "--model-i", "stem_roi_i", "--model-i-checkpoint", "a", "--model-p", "stem_roi",
                                             "--model-p-checkpoint", "b", "--input", "i", "--output", "o", "--width", "8", "--height", "6", "--level", "0.25",
                                             "--roi", "0,0,4,4,1", "--roi", "2,2,6,6,0.5,1", "--gop", "3", "--all-intra", "--bit-depth", "10"])
    assert (args.roi, args.level, args.gop, args.all_intra, args.bit_depth, args.roi_file) == (["0,0,4,4,1", "2,2,6,6,0.5,1"], 0.25, 3, True, 10, None)
    rois = video_pixel._cli_rois(args)
    assert rois(0) == rois(7) == [(0, 0, 4, 4, 1.0), (2, 2, 6, 6, 0.5, 1)]
    args = video_pixel._parser().parse_args(["decode", "--model-i", "stem_roi_i", "--model-i-checkpoint", "a", "--input", "i", "--output", "o", "--frames", "3:5"])
    assert args.frames == "3:5" and args.model_p is None


def test_the_command_line_refuses_with_a_status(models, tmp_path, capsys):
    ck_i, ck_p, ck_m = tmp_path / "i.pt", tmp_path / "p.pt", tmp_path / "m.pt"
    torch.save(models["roi_i"].state_dict(), ck_i)
    torch.save(models["roi"].state_dict(), ck_p)
    torch.save(models["mean"].state_dict(), ck_m)
    raw = tmp_path / "in.yuv"
    raw.write_bytes(bytes(2 * 6 * 4 * 3 // 2))                                         # two frames: the second one is a P frame
    roi_file = tmp_path / "rois.txt"
    roi_file.write_text("0 0 0 2 2 0.5\n1 0 0 2 2\n")
    io_ = ["--input", str(raw), "--output", str(tmp_path / "o"), "--device", "cpu"]
    mi = ["--model-i", "stem_roi_i", "--model-i-checkpoint", str(ck_i)]
    mp = ["--model-p", "stem_roi", "--model-p-checkpoint", str(ck_p)]
    size = ["--width", "4", "--height", "6"]
    main = video_pixel.main
    assert main(["encode", "--model-i", "nope", "--model-i-checkpoint", str(ck_i), *size, *io_]) == 2
    assert main(["encode", "--model-i", "stem_roi_i", "--model-i-checkpoint", str(ck_m), *size, *io_]) == 2        # not that model's checkpoint
    assert main(["encode", *mi, "--model-p", "stem_roi", *size, *io_]) == 2                                        # a class without a checkpoint
    assert main(["encode", *mi, "--model-p", "stem_roi_i", "--model-p-checkpoint", str(ck_i), *size, *io_]) == 2   # no P-frame class
    assert main(["encode", *mi, *mp, "--width", "5", "--height", "6", "--level", "0.5", *io_]) == 2                # odd side
    assert main(["encode", *mi, *size, "--level", "0.5", *io_]) == 2                                               # P frames, no P model
    assert main(["encode", *mi, *mp, *size, *io_]) == 2                                                            # no map for models that take one
    assert main(["encode", *mi, *mp, *size, "--roi", "0,0,2,2", *io_]) == 2
    assert main(["encode", *mi, *mp, *size, "--roi-file", str(roi_file), *io_]) == 2
    assert main(["encode", "--model-i", "mbt2018-mean", "--model-i-checkpoint", str(ck_m), "--all-intra", *size, "--level", "0.5", *io_]) == 2
    assert main(["decode", *mi, *mp, *io_]) == 2                                                                   # the .yuv is no sequence file
    assert main(["decode", *mi, *mp, "--frames", "3", *io_]) == 2
    err = capsys.readouterr().err
    assert err.count("refused") == 12
