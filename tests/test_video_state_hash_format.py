"""CPU: the state-hash trailer of the two sequence file formats (video.py, video_pixel.py): bit 7 of the version byte, `frames` big-endian
u64 behind the last record, records untouched.  Headers are built from their fields, strings are made up: nothing here runs a model."""
import struct

import pytest

from spatiotemporalentropymodel_amd import video, video_pixel

N, GOP = 7, 2
HASHES = [0, 1, 2 ** 64 - 1, 0x0123456789ABCDEF, 0xE220A8397B1DCDAF, 2 ** 63, 0xFFFFFFFF00000000]
COMMON = dict(width=104, height=120, bit_depth=8, frames=N, gop=GOP, all_intra=0, quality=4)
FIELDS = {"video": dict(COMMON, imodel_id=2, imodel_n=8, imodel_m=16, imodel_crc=0xDEADBEEF, stem_class=4, stem_n=8, stem_m=16, stem_crc=0x01020304),
          "video_pixel": dict(COMMON, i_kind=64, i_a=8, i_b=16, i_crc=0xDEADBEEF, p_kind=2, p_a=8, p_b=16, p_crc=0x01020304)}
MODULES = {"video": video, "video_pixel": video_pixel}


def _strings(k):
    return [[bytes([k, 1, 2, 3] * (k + 1))], [bytes([9, k])]]


def _records(name, hdr):
    if name == "video":
        return [video.record_bytes(hdr.imodel_name, 4, "raster", (120, 104), (2, 2), _strings(k)) for k in range(N)]
    return [video_pixel.record_bytes(hdr.record_byte(t), 4, (120, 104), (2, 2), _strings(k)) for k, t in enumerate(hdr.types())]


@pytest.fixture(params=sorted(MODULES))
def fmt(request):
    """(module, the un-hashed header, the hashed header, the records) of one format"""
    name = request.param
    mod = MODULES[name]
    plain, hashed = mod.FileHeader(**FIELDS[name]), mod.FileHeader(state_hash=True, **FIELDS[name])
    return mod, plain, hashed, _records(name, plain)


def test_the_flag_is_bit_7_of_the_version_byte_and_nothing_else(fmt):
    mod, plain, hashed, _ = fmt
    assert video.STATE_HASH_BIT == 0x80 and mod.VERSION == 1 and mod.HEADER_BYTES == 42
    assert "state_hash" not in mod._FIELDS and len(mod._FIELDS) == 15
    assert plain.state_hash is False and hashed.state_hash is True
    a, b = plain.pack(), hashed.pack()
    assert a == mod._HEADER.pack(mod.MAGIC, 1, *plain.astuple())                       # an un-hashed header is today's bytes
    assert len(a) == len(b) == 42 and a[4] == 1 and b[4] == 0x81
    assert [i for i in range(42) if a[i] != b[i]] == [4]
    assert plain != hashed and plain.astuple() == hashed.astuple()
    assert mod.FileHeader.unpack(a) == plain and mod.FileHeader.unpack(b) == hashed
    assert mod.FileHeader.unpack(b).state_hash is True and mod.FileHeader.unpack(a).state_hash is False
    assert mod.FileHeader.unpack(b).pack() == b
    assert "state_hash" in repr(hashed) and "state_hash" not in repr(plain)


def test_both_headers_are_the_one_container_header(fmt):
    """one class states the struct; a format adds its magic and the names of its model fields.  The layout, written out: magic, version,
    w, h, bit depth, frames, gop, all_intra, quality, then per model a kind byte, two u16 and the u32 fingerprint"""
    from spatiotemporalentropymodel_amd import seqfile
    mod, plain, hashed, _ = fmt
    assert issubclass(mod.FileHeader, seqfile.FileHeader) and mod.FileHeader is not seqfile.FileHeader
    assert video.FileHeader is not video_pixel.FileHeader and mod._HEADER is seqfile._HEADER
    magic, i_kind, p_kind = (b"STMV", 2, 4) if mod is video else (b"STPX", 64, 2)
    want = struct.pack(">4sB" "IIBIIBB" "BHHI" "BHHI", magic, 1, 104, 120, 8, N, GOP, 0, 4, i_kind, 8, 16, 0xDEADBEEF, p_kind, 8, 16, 0x01020304)
    assert plain.pack() == want and hashed.pack() == want[:4] + b"\x81" + want[5:]
    other = video_pixel if mod is video else video
    with pytest.raises(ValueError, match="magic"):
        other.FileHeader.unpack(want)                                                   # a format reads its own files only


def test_a_broken_file_is_refused_before_the_models_are_looked_at(fmt):
    """the order of checks, the same in both codecs: the file's own consistency (it costs nothing), then the models.  A file cut inside
    its last record and a model of no known class: the truncation is what is reported"""
    mod, plain, hashed, recs = fmt
    no_model = object()
    for hdr, tail in ((plain, b""), (hashed, video.trailer_bytes(HASHES))):
        good = hdr.pack() + b"".join(recs) + tail
        cut = hdr.pack() + b"".join(recs)[:-1]                                          # one byte short, trailer gone with it
        for data in (cut, good[:mod.HEADER_BYTES + sum(len(r) for r in recs[:-1]) + 23]):
            with pytest.raises(ValueError, match="truncated"):
                mod.decode_sequence(no_model, no_model, data)
        with pytest.raises(ValueError, match="truncated"):
            mod.verify_sequence(no_model, no_model, cut)
        with pytest.raises(ValueError, match="none of"):                               # an intact file: now the models are what is wrong
            mod.decode_sequence(no_model, no_model, good)


@pytest.mark.parametrize("byte", [2, 0x82, 0, 0x80, 3, 0x41])
def test_other_versions_stay_refused(fmt, byte):
    mod, plain, _, _ = fmt
    data = plain.pack()
    with pytest.raises(ValueError, match="version"):
        mod.FileHeader.unpack(data[:4] + bytes([byte]) + data[5:])


def test_the_trailer_round_trips_and_the_records_are_the_unhashed_files(fmt):
    mod, plain, hashed, recs = fmt
    body = b"".join(recs)
    unhashed = plain.pack() + body
    trailer = video.trailer_bytes(HASHES)
    assert trailer == b"".join(struct.pack(">Q", v) for v in HASHES) and len(trailer) == 8 * N
    data = hashed.pack() + body + trailer
    assert data[:4] == unhashed[:4] and data[5:len(unhashed)] == unhashed[5:] and data[len(unhashed):] == trailer
    assert mod.read_state_hashes(data) == HASHES and mod.read_state_hashes(unhashed) is None
    assert mod.read_state_hashes(bytearray(data)) == HASHES
    want = video.record_ranges(unhashed, N, mod.HEADER_BYTES)
    assert video.record_ranges(data[:len(data) - 8 * N], N, mod.HEADER_BYTES) == want
    ranges, hashes = video.hashed_record_ranges(data, hashed, mod.HEADER_BYTES)
    assert ranges == want and hashes == HASHES and ranges[-1][1] == len(data) - 8 * N
    assert video.hashed_record_ranges(unhashed, plain, mod.HEADER_BYTES) == (want, None)
    assert video.split_trailer(data, hashed, mod.HEADER_BYTES) == (data[:len(unhashed)], HASHES)
    assert video.split_trailer(unhashed, plain, mod.HEADER_BYTES) == (unhashed, None)


def test_a_partial_decode_finds_its_entries_at_a_fixed_distance_from_the_end(fmt):
    """frames=(a, b) needs trailer entries a .. b: entry t sits 8 * (frames - t) bytes from the end, whatever the records hold"""
    mod, _, hashed, recs = fmt
    data = hashed.pack() + b"".join(recs) + video.trailer_bytes(HASHES)
    for a, b in ((3, 6), (0, 1), (6, 7), (0, 7)):
        assert mod.read_state_hashes(data)[a:b] == HASHES[a:b]
        assert [struct.unpack_from(">Q", data, len(data) - 8 * (N - t))[0] for t in range(a, b)] == HASHES[a:b]
    types = hashed.types()
    assert video.gop_starts(types) == [0, 0, 2, 2, 4, 4, 6]
    touched = sorted(i for step in video.decode_steps(types, 8, 3, 6) for i, _, _ in step)
    assert touched == [2, 3, 4, 5]                                                        # frame 2 is decoded, and checked, for the chain's sake


def test_short_long_and_misaligned_trailers_raise(fmt):
    mod, plain, hashed, recs = fmt
    body = b"".join(recs)
    good = hashed.pack() + body + video.trailer_bytes(HASHES)
    for bad in (good[:-1], good[:-8], good[:-8 * N], good[:-8 * N - 1], good + b"\0", good + b"\0" * 8, good[:-4], hashed.pack(),
                hashed.pack() + b"\0" * (8 * N - 1), hashed.pack() + video.trailer_bytes(HASHES)):
        with pytest.raises(ValueError):
            mod.read_state_hashes(bad)
        with pytest.raises(ValueError):
            video.hashed_record_ranges(bad, hashed, mod.HEADER_BYTES)
    with pytest.raises(ValueError, match="trailer"):
        mod.read_state_hashes(good[:-8])
    with pytest.raises(ValueError, match="trailer"):
        mod.read_state_hashes(good + b"\0" * 8)
    with pytest.raises(ValueError, match="trailer"):
        mod.read_state_hashes(hashed.pack() + b"\0" * 8)
    # an un-hashed file with bytes behind its last record is refused as today, also when they look like a trailer
    with pytest.raises(ValueError, match="behind the last"):
        mod.read_state_hashes(plain.pack() + body + video.trailer_bytes(HASHES))
    with pytest.raises(ValueError, match="behind the last"):
        video.record_ranges(plain.pack() + body + b"\0", N, mod.HEADER_BYTES)


def test_the_mismatch_error_carries_its_frame_its_gop_and_both_hashes():
    e = video.StateMismatch(5, 4, 0x0123456789ABCDEF, 0xE220A8397B1DCDAF)
    assert isinstance(e, ValueError) and (e.frame, e.gop_start, e.want, e.got) == (5, 4, 0x0123456789ABCDEF, 0xE220A8397B1DCDAF)
    text = str(e)
    assert "frame 5" in text and "frame 4" in text and "0123456789abcdef" in text and "e220a8397b1dcdaf" in text
    assert video_pixel.StateMismatch is video.StateMismatch


def test_the_command_lines_know_the_new_options():
    for mod, models in ((video, ["--imodel", "mbt2018-mean", "--imodel-checkpoint", "i.pt"]),
                        (video_pixel, ["--model-i", "stem_roi_i", "--model-i-checkpoint", "i.pt"])):
        p = mod._parser()
        enc = ["encode"] + models + ["--input", "a.yuv", "--output", "a.bin", "--width", "64", "--height", "64"]
        assert p.parse_args(enc).state_hash is False and p.parse_args(enc + ["--state-hash"]).state_hash is True
        dec = ["decode"] + models + ["--input", "a.bin", "--output", "a.yuv"]
        assert p.parse_args(dec).no_verify is False and p.parse_args(dec + ["--no-verify"]).no_verify is True
        ver = p.parse_args(["verify"] + models + ["--input", "a.bin"])
        assert ver.command == "verify" and not hasattr(ver, "output")
        with pytest.raises(SystemExit):
            p.parse_args(["verify"] + models + ["--input", "a.bin", "--output", "a.yuv"])


def test_the_report_prints_as_json_and_gives_the_exit_status(capsys):
    import json
    clean = {"frames": 7, "checked": 7, "mismatches": [], "unchecked": []}
    assert video.print_report(clean) == 0 and json.loads(capsys.readouterr().out) == clean
    bad = {"frames": 7, "checked": 6, "mismatches": [{"frame": 0, "gop_start": 0, "want": 1, "got": 2 ** 64 - 1}], "unchecked": [1]}
    assert video.print_report(bad) == 3
    out = json.loads(capsys.readouterr().out)
    assert out["mismatches"] == [{"frame": 0, "gop_start": 0, "want": "0000000000000001", "got": "ffffffffffffffff"}] and out["unchecked"] == [1]
