"""GPU, op level: the conditioning-state hash kernel (csrc/statehash.hip, include/stem_statehash.h) bit for bit against the numpy
statement in tests/state_hash_ref.py, in both layouts, dense and pitched, aligned for 16-byte loads and not, around the chunk size,
with sentinels around the output, a poisoned workspace and a relaunch.  Integers: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import state_hash_ref as R

pytestmark = pytest.mark.gpu
GUARD = 16
SENTINEL = 0x5A5A5A5A5A5A5A5A
POISON = -0x0123456789ABCDEF


def _chunk():
    from spatiotemporalentropymodel_amd import _lib
    return _lib.header_macro("stem_statehash.h", "STEM_STATE_HASH_CHUNK")


def _values(shape, seed, kind="mixed"):
    """random values with zeros of both signs and NaNs of two payloads among them; "zeros": +0.0 everywhere"""
    if kind == "zeros":
        return np.zeros(shape, dtype=np.float32)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    bits = flat.view(np.uint32)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    bits[5::13] = 0x7FC00001
    bits[2::17] = 0xFFC12345
    return x


def _planar(x, pad, off):
    """x [B,C,H,W] (numpy) as a planar device view with rows `pad` floats wider, starting `off` columns in (0, 0: dense)"""
    B, C, H, W = x.shape
    big = torch.full((B, C, H + 2, W + pad), 123.25, dtype=torch.float32, device="cuda")
    view = big[:, :, 1:1 + H, off:off + W]
    view.copy_(torch.from_numpy(x))
    return view


def _channels_last(x, pad, off):
    """the same as a channels-last device view with pixels `pad` floats wider, starting `off` channels in"""
    B, C, H, W = x.shape
    big = torch.full((B, H + 2, W + 2, C + pad), -77.5, dtype=torch.float32, device="cuda")
    view = big[:, 1:1 + H, 1:1 + W, off:off + C].permute(0, 3, 1, 2)
    view.copy_(torch.from_numpy(x))
    return view


def _shifted(x, channels_last):
    """x dense behind a base pointer one float past a 16-byte boundary"""
    B, C, H, W = x.shape
    flat = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    if channels_last:
        view = flat[1:].view(B, H, W, C).permute(0, 3, 1, 2)
    else:
        view = flat[1:].view(B, C, H, W)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4
    return view


def _variants(x):
    """(name, device view) of one logical tensor: both layouts, dense, with a pitch that keeps 16-byte alignment, with one that breaks
    it, and behind a shifted base pointer"""
    W, C = x.shape[3], x.shape[1]
    keep_w, keep_c = 4 + (-W) % 4, 4 + (-C) % 4                 # the padded extent is a multiple of 4 again
    return [("planar dense", torch.from_numpy(x).cuda()),
            ("planar pitch aligned", _planar(x, keep_w, 4)),
            ("planar pitch unaligned", _planar(x, keep_w + 1, 1)),
            ("planar shifted", _shifted(x, False)),
            ("channels-last dense", torch.from_numpy(x).cuda().contiguous(memory_format=torch.channels_last)),
            ("channels-last pitch aligned", _channels_last(x, keep_c, 4)),
            ("channels-last pitch unaligned", _channels_last(x, keep_c + 1, 1)),
            ("channels-last shifted", _shifted(x, True))]


@pytest.mark.parametrize("B", [1, 3], ids=lambda b: f"B{b}")
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (17, 5), (68, 120)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("C", [1, 3, 4, 6, 192], ids=lambda c: f"C{c}")
def test_bit_equal_to_the_reference_in_every_layout(C, hw, B):
    from spatiotemporalentropymodel_amd import functional as F
    x = _values((B, C) + hw, seed=C * 1000 + hw[0] * 10 + B)
    want = R.state_hash(x)
    assert len(set(want)) == B
    for name, view in _variants(x):
        assert tuple(view.shape) == x.shape
        got = F.state_hash(view)
        assert got.dtype == torch.int64 and tuple(got.shape) == (B,)
        assert F.state_hash_ints(got) == want, name


def _direct(t, strides, guard_ws=True):
    """the entry point itself on tensor t [B,C,H,W] with the given strides: out between sentinels, the workspace poisoned and followed
    by sentinels -> (hashes as ints, every sentinel survived, the workspace's size in words)"""
    from spatiotemporalentropymodel_amd import _lib
    from spatiotemporalentropymodel_amd import functional as F
    lib = _lib.statehash()
    B, C, H, W = t.shape
    need = lib.stem_state_hash_workspace_bytes(B, C, H, W)
    assert need % 8 == 0
    words = need // 8
    obuf = torch.full((B + 2 * GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    wbuf = torch.full((words + GUARD,), POISON, dtype=torch.int64, device="cuda")
    wbuf[words:] = SENTINEL
    out = obuf[GUARD:GUARD + B]
    _lib.check_statehash(lib.stem_state_hash(t.data_ptr(), B, C, H, W, *strides, out.data_ptr(), wbuf.data_ptr() if words else None, need,
                                             F._stream()))
    ok = bool((obuf[:GUARD] == SENTINEL).all()) and bool((obuf[GUARD + B:] == SENTINEL).all()) and bool((wbuf[words:] == SENTINEL).all())
    return F.state_hash_ints(out), ok, words


def _chunk_counts():
    c = _chunk()
    return [c - 1, c, c + 1, 2 * c + 3]


@pytest.mark.parametrize("layout", ["planar", "channels-last"])
@pytest.mark.parametrize("which", range(4), ids=["CHUNK-1", "CHUNK", "CHUNK+1", "2CHUNK+3"])
@pytest.mark.parametrize("kind", ["mixed", "zeros"])
def test_element_counts_around_the_chunk_with_sentinels_and_a_poisoned_workspace(which, layout, kind):
    """one row of n elements along the unit-stride dimension, B = 2: the last workgroup is partly empty, the hand-over between
    workgroups starts at CHUNK + 1, nothing outside out[0:B] and the workspace is written, and a relaunch gives the same bits"""
    n = _chunk_counts()[which]
    shape = (2, 1, 1, n) if layout == "planar" else (2, n, 1, 1)
    x = _values(shape, seed=n, kind=kind)
    want = R.state_hash(x)
    t = torch.from_numpy(x).cuda()
    strides = (n, n, n, 1) if layout == "planar" else (n, 1, n, n)
    got, ok, words = _direct(t, strides)
    assert words == (0 if n <= _chunk() else 2 * -(-n // _chunk()))
    assert ok and got == want
    again, ok2, _ = _direct(t, strides)
    assert ok2 and again == got


@pytest.mark.parametrize("shape", [(3, 6, 17, 5), (2, 4, 68, 120), (2, 192, 17, 5)], ids=str)
def test_sentinels_poison_and_relaunch_on_pitched_views(shape):
    x = _values(shape, seed=sum(shape))
    want = R.state_hash(x)
    for name, view in _variants(x):
        from spatiotemporalentropymodel_amd import functional as F
        strides = F.state_hash_strides(view.shape, view.stride())
        got, ok, _ = _direct(view, strides)
        assert ok and got == want, name
        again, ok2, _ = _direct(view, strides)
        assert ok2 and again == got, name


def test_out_as_a_slice_of_a_longer_buffer_and_the_gaps_of_a_view_are_not_hashed():
    from spatiotemporalentropymodel_amd import functional as F
    x = _values((2, 4, 17, 8), seed=9)
    y = _values((1, 3, 40, 50), seed=10)
    buf = torch.full((7,), SENTINEL, dtype=torch.int64, device="cuda")
    r0 = F.state_hash(torch.from_numpy(x).cuda(), out=buf[1:3])
    r1 = F.state_hash(torch.from_numpy(y).cuda(), out=buf[4:5])
    assert r0.data_ptr() == buf[1:3].data_ptr() and r1.data_ptr() == buf[4:5].data_ptr()
    ints = F.state_hash_ints(buf)
    assert ints[1:3] == R.state_hash(x) and ints[4:5] == R.state_hash(y)
    assert [ints[k] for k in (0, 3, 5, 6)] == [SENTINEL] * 4
    view = _planar(x, 4, 4)
    before = F.state_hash_ints(F.state_hash(view))
    big = torch.full((2, 4, 19, 12), 5.0, dtype=torch.float32, device="cuda")            # other values in the gaps: the same hash
    big[:, :, 1:18, 4:12] = torch.from_numpy(x).cuda()
    assert F.state_hash_ints(F.state_hash(big[:, :, 1:18, 4:12])) == before == R.state_hash(x)
    for bad in (buf[1:4], buf[::2][:2], buf[1:3].to(torch.int32), buf[1:3].cpu()):
        with pytest.raises(ValueError, match="out="):
            F.state_hash(torch.from_numpy(x).cuda(), out=bad)


def test_a_single_changed_bit_and_a_swap_change_the_hash():
    from spatiotemporalentropymodel_amd import functional as F
    x = _values((1, 192, 17, 5), seed=3)
    t = torch.from_numpy(x).cuda().contiguous(memory_format=torch.channels_last)
    base = F.state_hash_ints(F.state_hash(t))
    u = t.clone()
    u.view(torch.int32)[0, 100, 9, 2] ^= 1                                              # one ulp somewhere
    v = t.clone()
    a, b = t[0, 7, 3, 1].item(), t[0, 8, 3, 1].item()
    assert a != b
    v[0, 7, 3, 1], v[0, 8, 3, 1] = b, a
    hu, hv = F.state_hash_ints(F.state_hash(u)), F.state_hash_ints(F.state_hash(v))
    assert len({base[0], hu[0], hv[0]}) == 3
    assert hu == R.state_hash(u.cpu().numpy()) and hv == R.state_hash(v.cpu().numpy())
