"""The dropout keep-mask of the kernels (csrc/common.h drop_init / drop_keep / drop_keep_at) restated in numpy integer arithmetic,
bit-exact with the device code: keep(idx) is a pure counter hash of (device seed, site salt, flat element index of the site's
LOGICAL tensor).  tests/test_dropout_parity_gpu.py builds every ground-truth mask from here, never from a kernel's output."""
import numpy as np

M32 = 0xFFFFFFFF
DROP_HI_MUL = 0x9E3779B1


def mix32(x):
    """lowbias32."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def keys(seed, salt):
    """(k0, k1) of drop_init: the seed's low word XOR salt * 0x9E3779B9, its high word + salt * 0x85EBCA6B + 0x165667B1, each through
    the mixer.  The salt is a uint32 (ops._drop masks it), the seed any 64-bit integer (the device holds it as int64)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    salt = int(salt) & M32
    k0 = mix32((seed & M32) ^ ((salt * 0x9E3779B9) & M32))
    k1 = mix32(((seed >> 32) + salt * 0x85EBCA6B + 0x165667B1) & M32)
    return int(k0), int(k1)


def thresh(p):
    """uint32(float32(p) * float32(2^24)): p is rounded to float32 FIRST (the descriptor carries a float).  The product itself is
    exact (a power of two), so float32 and float64 arithmetic on the rounded p agree; float64 `p * 2**24` on the unrounded p does
    not always: p = 0.6 gives 10066329 there and 10066330 here (float32(0.6) = 0.60000002384 lies above 0.6)."""
    return int(np.uint32(np.float32(p) * np.float32(16777216.0)))


def scale(p):
    """1 / (1 - p) as the kernels compute it: float32 throughout."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def drop_keep(k0, k1, th, idx):
    """keep(idx) = (mix32((lo(idx) ^ k0) + hi(idx) * DROP_HI_MUL + k1) >> 8) >= thresh for 64-bit indices (array or scalar)."""
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = idx & M32, idx >> 32
    r = mix32(((lo ^ k0) + ((hi * DROP_HI_MUL) & M32) + k1) & M32)
    return (r >> 8) >= th


def drop_keep_at(k0, k1, th, base, off):
    """The same for idx = base + off with a (wave-uniform) 64-bit base and 32-bit offsets, as the device computes it: the high word's
    term is prepared once from the base, and a carry out of the low word adds DROP_HI_MUL once more."""
    base = int(base) & 0xFFFFFFFFFFFFFFFF
    off = np.asarray(off, dtype=np.uint64) & M32
    b_lo, b_hic = base & M32, ((base >> 32) * DROP_HI_MUL) & M32
    lo = (b_lo + off) & M32
    carry = np.where(lo < b_lo, np.uint64(DROP_HI_MUL), np.uint64(0))
    r = mix32(((lo ^ k0) + ((b_hic + k1) & M32) + carry) & M32)
    return (r >> 8) >= th


def keep_mask(seed, salt, p, n, start=0):
    """bool[n]: the keep bits of elements start .. start + n - 1 of site `salt` under device seed `seed`.  p = 0: dropout is off,
    everything is kept (the kernels do not hash at all then)."""
    if not p > 0.0:
        return np.ones(int(n), dtype=bool)
    k0, k1 = keys(seed, salt)
    idx = np.uint64(int(start)) + np.arange(int(n), dtype=np.uint64)
    return drop_keep(k0, k1, thresh(p), idx)
