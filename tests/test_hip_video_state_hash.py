"""GPU, model level: per-frame state hashes of the latent-domain sequence codec (video.py) on the 7-frame, 120 x 104, gop = 2 sequence
and the models of tests/test_hip_video.py.  The hashed file is the un-hashed one plus a bit and a trailer; the trailer holds
functional.state_hash of every frame's y_hat; the decoder checks it before a state becomes a condition; verify_sequence checks a file
on latents alone.  A decoder is never fed a stream it was not made for: a divergent state is produced by putting another sequence's
(valid, self-contained) I record in place of the first one, or by changing the trailer -- no string is damaged, none is decoded under
foreign priors."""
import io

import pytest
import torch

from test_hip_video import DEV, gop_models, golden_frames                              # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
N, GOP, H, W = 7, 2, 120, 104
FRAME_BYTES = H * W * 3 // 2


@pytest.fixture(scope="module")
def frames(golden_frames):
    from test_hip_encode_batch import _sequence
    out = _sequence(golden_frames)
    assert len(out) == N and tuple(out[0].shape) == (3, H, W)
    return out


def _encode(models, frames, **kw):
    from spatiotemporalentropymodel_amd import video
    buf = io.BytesIO()
    res = video.encode_sequence(*models, frames, buf, gop=GOP, **kw)
    return buf.getvalue(), res


@pytest.fixture(scope="module")
def coded(gop_models, frames):
    """the sequence coded once without and once with hashes (raster, three GOPs side by side), and a second sequence B of the same
    geometry (the frames mirrored), hashed too"""
    plain, _ = _encode(gop_models, frames, concurrent_gops=3)
    hashed, res = _encode(gop_models, frames, concurrent_gops=3, state_hash=True)
    other, _ = _encode(gop_models, [f.flip(-1).contiguous() for f in frames], concurrent_gops=3, state_hash=True)
    return {"plain": plain, "hashed": hashed, "res": res, "other": other}


@pytest.fixture(scope="module")
def decoded(gop_models, coded):
    """the un-hashed decode, computed once and left alone: (frames, .yuv bytes)"""
    from spatiotemporalentropymodel_amd import video
    sink = io.BytesIO()
    return video.decode_sequence(*gop_models, coded["plain"], write_to=sink), sink.getvalue()


@pytest.mark.parametrize("order", ["raster", "wavefront"])
@pytest.mark.parametrize("concurrent", [1, 3])
def test_header_and_records_are_the_unhashed_files(gop_models, frames, concurrent, order):
    from spatiotemporalentropymodel_amd import video
    plain, res0 = _encode(gop_models, frames, concurrent_gops=concurrent, order=order)
    hashed, res1 = _encode(gop_models, frames, concurrent_gops=concurrent, order=order, state_hash=True)
    assert plain[4] == 1 and hashed[4] == 0x81
    assert len(hashed) == len(plain) + 8 * N and hashed[:4] == plain[:4] and hashed[5:len(plain)] == plain[5:]
    assert "state_hash" not in res0 and res0["bytes"] == len(plain)
    assert res1["bytes"] == len(hashed) and res1["frames"] == res0["frames"] and res1["bpp_ave"] == res0["bpp_ave"]
    assert res1["state_hash"] == video.read_state_hashes(hashed) and len(res1["state_hash"]) == N
    h = res1["state_hash"]
    assert h[0] == h[6] and len(set(h)) == N - 1                                       # frame 6 is frame 0 again, both I frames: equal states, equal hashes
    assert video.read_state_hashes(plain) is None
    assert hashed[len(plain):] == video.trailer_bytes(res1["state_hash"])


def test_the_trailer_holds_the_hash_of_every_frames_y_hat(gop_models, coded, monkeypatch):
    """entry t is functional.state_hash of the y_hat decode_sequence holds for frame t (the un-hashed file: nothing is verified here)"""
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd import video
    held, inner = {}, video._decode_step

    def spy(imodel, stem, hdr, step, recs, y_cond, **kw):
        y_hat, x_hat = inner(imodel, stem, hdr, step, recs, y_cond, **kw)
        for (index, _, _), y in zip(step, y_hat):
            held[index] = y
        return y_hat, x_hat

    monkeypatch.setattr(video, "_decode_step", spy)
    video.decode_sequence(*gop_models, coded["plain"], return_frames=False)
    assert sorted(held) == list(range(N))
    want = video.read_state_hashes(coded["hashed"])
    for t in range(N):
        assert held[t].dim() == 4 and held[t].shape[0] == 1
        assert F.state_hash_ints(F.state_hash(held[t])) == [want[t]], f"frame {t}"
    assert coded["res"]["state_hash"] == want


@pytest.mark.parametrize("concurrent", [1, 3])
def test_a_clean_hashed_file_decodes_to_the_unhashed_decode(gop_models, coded, decoded, concurrent):
    from spatiotemporalentropymodel_amd import video
    sink = io.BytesIO()
    got = video.decode_sequence(*gop_models, coded["hashed"], write_to=sink, concurrent_gops=concurrent)
    assert len(got) == N and all(torch.equal(a, b) for a, b in zip(got, decoded[0]))
    assert sink.getvalue() == decoded[1] and len(decoded[1]) == N * FRAME_BYTES


def test_verify_false_an_unhashed_file_and_a_plain_encode_hash_nothing(gop_models, frames, coded, decoded, monkeypatch):
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd import video

    def trap(*a, **k):
        raise AssertionError("state_hash ran")

    monkeypatch.setattr(F, "state_hash", trap)
    for data, kw in ((coded["hashed"], {"verify": False}), (coded["plain"], {}), (coded["plain"], {"verify": True})):
        got = video.decode_sequence(*gop_models, data, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, decoded[0]))
    assert _encode(gop_models, frames, concurrent_gops=3)[0] == coded["plain"]
    with pytest.raises(AssertionError, match="state_hash ran"):
        _encode(gop_models, frames[:1], state_hash=True)


def _trap_synthesis(monkeypatch, imodel):
    calls = []

    def trap(name):
        def fn(*a, **k):
            calls.append(name)
            raise AssertionError(f"{name} was called while verifying")
        return fn

    monkeypatch.setattr(imodel, "getX", trap("imodel.getX"), raising=False)
    hook = imodel.g_s.register_forward_pre_hook(lambda *a: trap("imodel.g_s")())
    return calls, hook


@pytest.mark.parametrize("concurrent", [1, 8])
def test_verify_sequence_checks_every_frame_on_latents_alone(gop_models, coded, monkeypatch, concurrent):
    from spatiotemporalentropymodel_amd import video
    calls, hook = _trap_synthesis(monkeypatch, gop_models[0])
    try:
        report = video.verify_sequence(*gop_models, coded["hashed"], concurrent_gops=concurrent)
    finally:
        hook.remove()
    assert calls == []
    assert report == {"frames": N, "checked": N, "mismatches": [], "unchecked": []}
    with pytest.raises(ValueError, match="no state hashes"):
        video.verify_sequence(*gop_models, coded["plain"])


def test_a_partial_decode_verifies_and_is_a_slice(gop_models, coded, decoded, monkeypatch):
    from spatiotemporalentropymodel_amd import video
    hashed_frames, inner = [], video._hash_states

    def spy(states):
        out = inner(states)
        hashed_frames.append(len(out))
        return out

    monkeypatch.setattr(video, "_hash_states", spy)
    sink = io.BytesIO()
    got = video.decode_sequence(*gop_models, coded["hashed"], write_to=sink, frames=(3, 6))
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, decoded[0][3:6]))
    assert sink.getvalue() == decoded[1][3 * FRAME_BYTES:6 * FRAME_BYTES]
    assert sum(hashed_frames) == 4                                                      # frames 2 .. 5: frame 2 for the chain's sake, checked too


def _swap_first_record(coded):
    """A's header, B's first I record in place of A's, A's other records, A's trailer: every record is a valid stream of these models"""
    from spatiotemporalentropymodel_amd import video
    a, b = coded["hashed"], coded["other"]
    ra, _ = video.hashed_record_ranges(a, video.FileHeader.unpack(a))
    rb, _ = video.hashed_record_ranges(b, video.FileHeader.unpack(b))
    assert a[ra[0][0]:ra[0][1]] != b[rb[0][0]:rb[0][1]]
    return a[:ra[0][0]] + b[rb[0][0]:rb[0][1]] + a[ra[0][1]:]


def _count_stem_decodes(monkeypatch):
    from spatiotemporalentropymodel_amd import codec
    calls = []
    for name in ("stem_decompress", "stem_decompress_each"):
        inner = getattr(codec, name)
        monkeypatch.setattr(codec, name, (lambda inner, name: lambda *a, **k: (calls.append(name), inner(*a, **k))[1])(inner, name))
    return calls


@pytest.mark.parametrize("concurrent", [1, 3])
def test_a_foreign_first_record_is_caught_before_any_p_frame_of_its_chain(gop_models, coded, monkeypatch, concurrent):
    from spatiotemporalentropymodel_amd import video
    bad = _swap_first_record(coded)
    want = video.read_state_hashes(coded["hashed"])
    calls = _count_stem_decodes(monkeypatch)
    with pytest.raises(video.StateMismatch) as info:
        video.decode_sequence(*gop_models, bad, concurrent_gops=concurrent)
    e = info.value
    assert (e.frame, e.gop_start, e.want) == (0, 0, want[0]) and e.got == video.read_state_hashes(coded["other"])[0] != e.want
    assert "frame 0" in str(e) and f"{e.want:016x}" in str(e) and f"{e.got:016x}" in str(e)
    assert calls == []                                                                  # no P frame was decoded: the state never became a condition


@pytest.mark.parametrize("concurrent", [1, 8])
def test_verify_sequence_abandons_the_gop_and_checks_the_others(gop_models, coded, monkeypatch, concurrent):
    from spatiotemporalentropymodel_amd import video
    bad = _swap_first_record(coded)
    want = video.read_state_hashes(coded["hashed"])
    calls = _count_stem_decodes(monkeypatch)
    report = video.verify_sequence(*gop_models, bad, concurrent_gops=concurrent)
    assert report == {"frames": N, "checked": N - 1, "unchecked": [1],
                      "mismatches": [{"frame": 0, "gop_start": 0, "want": want[0], "got": video.read_state_hashes(coded["other"])[0]}]}
    assert len(calls) >= 1                                                              # the P frames of the other GOPs were decoded and checked


@pytest.mark.parametrize("k", [0, 3, 4])
def test_one_flipped_trailer_bit_reports_exactly_that_frame(gop_models, coded, k):
    from spatiotemporalentropymodel_amd import video
    good = coded["hashed"]
    bad = bytearray(good)
    bad[len(good) - 8 * (N - k) + 5] ^= 0x10
    bad = bytes(bad)
    want = video.read_state_hashes(good)
    flipped = video.read_state_hashes(bad)
    assert [t for t in range(N) if want[t] != flipped[t]] == [k]
    report = video.verify_sequence(*gop_models, bad)
    assert report["mismatches"] == [{"frame": k, "gop_start": k - k % GOP, "want": flipped[k], "got": want[k]}]
    assert report["unchecked"] == ([k + 1] if k % GOP == 0 and k + 1 < N else []) and report["checked"] == N - len(report["unchecked"])
    with pytest.raises(video.StateMismatch) as info:
        video.decode_sequence(*gop_models, bad)
    assert (info.value.frame, info.value.gop_start, info.value.want, info.value.got) == (k, k - k % GOP, flipped[k], want[k])
