"""The sensor-noise stage (`sd_noise_u8`, csrc/sd_noise.hip) restated in numpy, integers only -- what the kernel has to give byte for byte:

    o        = (y W + x) 3 + c, the byte's offset inside its image
    word(o)  = Philox4x32-10(counter (o >> 2, 0, 0, 0), key (k0, k1))[o & 3]
    z        = H[i - 2048] if i >= 2048 else -H[2047 - i],  i = word >> 20,  H[j] = round(1024 Phi^-1((2048 + j + 0.5) / 4096))
    sigma(v) = isqrt(min(a, 2^26) + min(b, 2^17) v), a and b the row's third and fourth words as uint32
    out      = clamp(v + ((z sigma(v) + 2^17) >> 18), 0, 255)

Philox is the generator of Salmon et al. (Random123), pinned by its published known-answer vectors in tests/test_noise_cpu.py."""
import functools
import math
from statistics import NormalDist

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57                                      # multipliers on counter words 0 and 2
W0, W1 = 0x9E3779B9, 0xBB67AE85                                      # key increments
MAX_A, MAX_B = 1 << 26, 1 << 17                                      # the clamps of a row's variance words
KINDS = ["zeros", "full", "ramp", "random"]
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two 32-bit ints -> four uint32 arrays, ten rounds; products in uint64."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


@functools.lru_cache(maxsize=None)
def half_table():
    """H[0 .. 2047], computed afresh from Python's statistics.NormalDist."""
    inv = NormalDist().inv_cdf
    h = np.asarray([int(round(1024.0 * inv((2048 + j + 0.5) / 4096.0))) for j in range(2048)], dtype=np.int64)
    h.setflags(write=False)
    return h


def isqrt(x):
    """The exact floor square root of non-negative integers (Python's math.isqrt, element by element)."""
    return np.asarray([math.isqrt(int(v)) for v in np.asarray(x).reshape(-1)], dtype=np.int64).reshape(np.shape(x))


def clamped(row):
    """(k0, k1, a', b') of a row of four integers of any sign: 32-bit patterns, the variance words clamped."""
    k0, k1, a, b = (int(v) & 0xFFFFFFFF for v in row)
    return k0, k1, min(a, MAX_A), min(b, MAX_B)


def sigma_table(row):
    _, _, a, b = clamped(row)
    return isqrt(a + b * np.arange(256, dtype=np.int64))


def unit_normals(n_bytes, key):
    """z of the bytes 0 .. n_bytes - 1 of an image, Q10, int64."""
    groups = (n_bytes + 3) // 4
    words = np.stack(philox4x32_10((np.arange(groups, dtype=np.uint64), 0, 0, 0), key), axis=1).reshape(-1)[:n_bytes]
    i = (words >> np.uint32(20)).astype(np.int64)
    h = half_table()
    return np.where(i >= 2048, h[np.maximum(i - 2048, 0)], -h[np.maximum(2047 - i, 0)])


def noise_ref(img, row):
    """img: (H, W, 3) uint8; row: [k0, k1, a, b] -> the noised image, uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.shape[0] * img.shape[1] < 2 ** 31
    k0, k1, a, b = clamped(row)
    v = img.reshape(-1).astype(np.int64)
    z = unit_normals(v.size, (k0, k1))
    n = (z * sigma_table(row)[v] + (1 << 17)) >> 18                  # numpy's >> on int64 is arithmetic
    return np.clip(v + n, 0, 255).astype(np.uint8).reshape(img.shape)


def rows_of(draws):
    """[k0, k1, round(sigma^2 65536), round(gain 65536)] of draws (k0, k1, sigma_read, gain), as plain non-negative integers."""
    return [[int(k0), int(k1), int(round(s * s * 65536.0)), int(round(g * 65536.0))] for k0, k1, s, g in draws]


def noise_image(kind, h, w, rng):
    """constant 0, constant 255, a ramp through all 256 values (every sigma-table entry matters; byte o holds o mod 256 shifted by a
    random start), or random bytes."""
    if kind == "zeros":
        return np.zeros((h, w, 3), dtype=np.uint8)
    if kind == "full":
        return np.full((h, w, 3), 255, dtype=np.uint8)
    if kind == "ramp":
        return ((np.arange(h * w * 3) + int(rng.integers(0, 256))) % 256).astype(np.uint8).reshape(h, w, 3)
    assert kind == "random", kind
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
