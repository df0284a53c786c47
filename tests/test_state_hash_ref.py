"""CPU: the numpy statement of the conditioning-state hash (tests/state_hash_ref.py) against a restatement in Python integers, its known
answers, and the properties the codecs lean on: the hash is a function of the values at their logical positions (not of the layout), it
is sensitive to position, and it is a plain sum over any split of the index range."""
import numpy as np
import pytest

import state_hash_ref as R


def _random(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    if flat.size > 5:
        flat.view(np.uint32)[5] = 0x7FC00001                   # two NaN payloads
        flat.view(np.uint32)[2] = 0xFFC12345
    return x


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 4, 5), (1, 6, 2, 3), (3, 4, 1, 7)], ids=str)
def test_numpy_equals_python_integers(shape):
    x = _random(shape, sum(shape))
    assert R.state_hash(x) == R.state_hash_int(x)
    assert all(0 <= v < 2 ** 64 for v in R.state_hash(x))


def test_mix64_is_splitmix64():
    """the first outputs of SplitMix64 seeded with 0 are mix64(0), mix64(golden), ...: the published sequence"""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [R.mix64_int((k * R.GOLDEN) & R.MASK) for k in range(3)] == want
    assert [int(v) for v in R.mix64(np.array([(k * R.GOLDEN) & R.MASK for k in range(3)], dtype=np.uint64))] == want


@pytest.mark.parametrize("values,shape,want", R.KNOWN, ids=[f"{k[2]:016X}" for k in R.KNOWN])
def test_known_answers(values, shape, want):
    x = np.array(values, dtype=np.float32).reshape((1,) + shape)
    assert R.state_hash(x) == [want] and R.state_hash_int(x) == [want]


def test_known_answer_arange6_in_the_issues_shape():
    assert R.state_hash(np.arange(6, dtype=np.float32).reshape(1, 2, 1, 3)) == [0x69EE030164F69B13]


def test_zero_signs_and_nan_payloads_differ():
    def one(bits):
        return R.state_hash(np.array([bits], dtype=np.uint32).view(np.float32).reshape(1, 1, 1, 1))[0]
    assert len({one(0x00000000), one(0x80000000), one(0x7FC00000), one(0x7FC00001), one(0xFFC00000)}) == 5


def test_layout_independence():
    x = _random((2, 6, 5, 7), 1)
    want = R.state_hash(x)
    nhwc = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).transpose(0, 3, 1, 2)                 # channels-last memory, NCHW view
    assert nhwc.strides != x.strides and R.state_hash(nhwc) == want
    big = np.full((2, 6, 9, 10), np.float32(7.5), dtype=np.float32)                              # a pitched planar view
    big[:, :, 2:7, 1:8] = x
    assert R.state_hash(big[:, :, 2:7, 1:8]) == want
    bigl = np.full((2, 5, 9, 8), np.float32(-3.0), dtype=np.float32)                             # a pitched channels-last view
    bigl[:, :, 1:8, 2:8] = x.transpose(0, 2, 3, 1)
    assert R.state_hash(bigl[:, :, 1:8, 2:8].transpose(0, 3, 1, 2)) == want


def test_position_sensitivity():
    x = _random((1, 3, 4, 5), 2)
    flat = x.reshape(-1)
    i, j = 8, 31
    assert flat.view(np.uint32)[i] != flat.view(np.uint32)[j]
    y = x.copy()
    yf = y.reshape(-1)
    yf[i], yf[j] = flat[j], flat[i]
    assert sorted(yf.view(np.uint32).tolist()) == sorted(flat.view(np.uint32).tolist())
    assert R.state_hash(y) != R.state_hash(x)


@pytest.mark.parametrize("cut", [0, 1, 17, 59, 60])
def test_additivity_over_a_split_of_the_index_range(cut):
    x = _random((1, 3, 4, 5), 3)
    bits = x.reshape(-1).view(np.uint32)
    with np.errstate(over="ignore"):
        left = int(np.sum(R.terms(bits[:cut], 0), dtype=np.uint64))
        right = int(np.sum(R.terms(bits[cut:], cut), dtype=np.uint64))
    assert (left + right) & R.MASK == R.state_hash(x)[0]
