"""tests/dropout_refs.py against itself: the properties the GPU parity tests rely on, and the one form of the hash that no
affordable GPU shape reaches (drop_keep_at with an index above 2^32)."""
import numpy as np
import pytest

from tests import dropout_refs as R

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _mix_py(x):
    """lowbias32 on python integers (no numpy: catches a wrap-around slip of the array form)."""
    x &= M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32
    x ^= x >> 15; x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def _keep_py(seed, salt, p, idx):
    seed &= M64; salt &= M32
    k0 = _mix_py((seed & M32) ^ ((salt * 0x9E3779B9) & M32))
    k1 = _mix_py((seed >> 32) + salt * 0x85EBCA6B + 0x165667B1)
    r = _mix_py(((idx & M32) ^ k0) + (idx >> 32) * 0x9E3779B1 + k1)
    return (r >> 8) >= int(np.float32(p) * np.float32(2.0 ** 24))


def test_array_form_equals_the_scalar_definition():
    assert int(R.mix32(0)) == 0 and int(R.mix32(1)) == _mix_py(1)
    for seed, salt, p in ((0x1234567812345678, 17, 0.1), (0xFFFFFFFF00000000, 0x80000003, 0.5), (-5, 6, 0.3), (77, 4 * 65 + 2, 0.25)):
        for start in (0, (1 << 32) - 8, (5 << 32) + 123):
            got = R.keep_mask(seed, salt, p, 16, start=start)
            want = [_keep_py(seed, salt, p, start + i) for i in range(16)]
            assert got.tolist() == want, (seed, salt, p, start)


@pytest.mark.parametrize("base", [(1 << 32) - 5, 1 << 32, (1 << 32) + 7, (3 << 32) - 1, 3 << 32, (3 << 32) + 0xFFFFFFF0, 0, 12345,
                                  (0xFFFFFFFF << 32) + 0xFFFFFFFE])
def test_drop_keep_at_is_drop_keep_of_the_sum(base):
    """Bases just below, at and above multiples of 2^32; offsets that stay inside the low word and offsets that carry out of it
    (including the largest 32-bit offset)."""
    k0, k1 = R.keys(0x0BADC0DE12345, 33)
    th = R.thresh(0.5)
    off = np.concatenate([np.arange(0, 40), np.arange(0xFFFFFFFF - 40, 0xFFFFFFFF + 1), np.array([1 << 31, (1 << 31) + 3, 0x12345678])]).astype(np.uint64)
    lo = (base & M32) + off
    assert bool((lo > M32).any()) or (base & M32) == 0                     # every base but the aligned ones sees a carry
    assert bool((lo <= M32).any())
    want = R.drop_keep(k0, k1, th, (np.uint64(base) + off) & np.uint64(M64))
    got = R.drop_keep_at(k0, k1, th, base, off)
    assert np.array_equal(got, want)
    assert 0.3 < got.mean() < 0.7                                          # not a constant


def test_the_high_word_of_the_seed_and_of_the_index_enter_the_hash():
    n = 1 << 12
    a = R.keep_mask(0x0000000112345678, 17, 0.5, n)
    b = R.keep_mask(0x0000000212345678, 17, 0.5, n)
    c = R.keep_mask(0x0000000112345679, 17, 0.5, n)
    for other in (b, c):
        assert 0.4 < (a != other).mean() < 0.6                             # independent fair coins differ half the time
    assert 0.4 < (a != R.keep_mask(0x0000000112345678, 17, 0.5, n, start=1 << 32)).mean() < 0.6


def test_salt_wraps_as_uint32():
    """ops._drop passes salt & 0xFFFFFFFF; a salt >= 2^31 must not be sign-extended, and salt and salt + 2^32 are one site."""
    n = 1 << 12
    big = 0x80000000 + 4 * 7 + 1
    a = R.keep_mask(99, big, 0.5, n)
    assert np.array_equal(a, R.keep_mask(99, big + (1 << 32), 0.5, n))
    assert np.array_equal(a, R.keep_mask(99, big - (1 << 32), 0.5, n))     # the same bits read as a negative int32
    assert 0.4 < (a != R.keep_mask(99, 4 * 7 + 1, 0.5, n)).mean() < 0.6   # bit 31 of the salt matters
    assert a.tolist() == [_keep_py(99, big, 0.5, i) for i in range(n)]


def test_threshold_and_scale_use_float32():
    """thresh rounds p to float32 before the (exact) multiplication by 2^24; float64 arithmetic on the unrounded p differs, e.g. at
    p = 0.6.  scale is the float32 quotient."""
    assert R.thresh(0.6) == 10066330 and int(0.6 * 2 ** 24) == 10066329
    for p in (0.1, 0.25, 0.3, 0.5, 0.6):
        assert R.thresh(p) == int(float(np.float32(p)) * 2 ** 24)
    assert R.thresh(0.1) == 1677721 and R.thresh(0.5) == 1 << 23
    assert R.scale(0.5) == np.float32(2.0) and R.scale(0.5).dtype == np.float32
    assert R.scale(0.1) == np.float32(1.0) / np.float32(0.9) and float(R.scale(0.1)) != 1.0 / 0.9


def test_p_zero_keeps_everything():
    assert R.keep_mask(123, 5, 0.0, 1000).all()
    k0, k1 = R.keys(123, 5)
    assert R.drop_keep(k0, k1, R.thresh(0.0), np.arange(1000)).all()     # threshold 0: the comparison itself keeps all


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_rate(p):
    n = 1 << 20
    rate = R.keep_mask(0x1234567812345678, 17, p, n).mean()
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(rate - (1 - p)) < 5 * sigma, (rate, sigma)
