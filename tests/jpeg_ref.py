"""Numpy restatement of Pillow's JPEG round trip `Image.save(buf, "JPEG", quality=q)` then `Image.open(buf)` on an RGB image whose sides
are multiples of 16 (libjpeg-turbo, 4:2:0, accurate-integer DCT), the reference the JPEG kernels are held to byte for byte.  It is pinned
against Pillow itself in tests/test_jpeg_cpu.py; the GPU tests compare `sd_jpeg_u8` with this file, never with the library's own host code.

The entropy coder is lossless, so the round trip is: RGB -> YCbCr (jccolor), chroma h2v2 downsample (jcsample), forward DCT "islow" on
sample - 128 (jfdctint: rows, then columns), quantise and dequantise, inverse DCT "islow" (jidctint: columns, then rows, range limit by
mask), chroma h2v2 "fancy" upsample (jdsample), YCbCr -> RGB (jdcolor).  All of it is signed 32-bit integer arithmetic with arithmetic
right shifts; the int64 arrays below assert that nothing leaves that range.
"""
import numpy as np

# Annex K of the JPEG standard, natural (row-major) order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                      72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32, dtype=np.int64).reshape(8, 8)

F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def jpeg_quant_tables(quality):
    """(ql, qc) of jpeg_set_quality(quality, force_baseline): 8 x 8 int arrays in natural order."""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def _i32(x):
    assert x.min() >= -(1 << 31) and x.max() < (1 << 31)
    return x


def _descale(x, n):
    return _i32(x + (1 << (n - 1))) >> n


def _odd(t4, t5, t6, t7):
    """The odd part shared by both transforms: -> (a, b, c, d)."""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2 = z1 * -F_0_899, z2 * -F_2_562
    z3, z4 = z3 * -F_1_961 + z5, z4 * -F_0_390 + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def _fdct_pass(d, first):
    """d: (..., 8) along the last axis -> (..., 8)."""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = _descale(z1 + t13 * F_0_765, n)
    o[6] = _descale(z1 - t12 * F_1_847, n)
    a, b, c, e = _odd(t4, t5, t6, t7)
    o[7], o[5], o[3], o[1] = _descale(a, n), _descale(b, n), _descale(c, n), _descale(e, n)
    return np.stack(o, axis=-1)


def _idct_pass(i, first):
    i = [i[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * F_0_541
    t2, t3 = z1 - i[6] * F_1_847, z1 + i[2] * F_0_765
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = _odd(i[7], i[5], i[3], i[1])
    n = 11 if first else 18
    o = [t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d]
    return np.stack([_descale(v, n) for v in o], axis=-1)


def _range_limit(x):
    m = x & 1023
    return np.where(m < 128, m + 128, np.where(m < 512, 255, np.where(m < 896, 0, m - 896)))


def _code_plane(p, q):
    """(h, w) samples, h and w multiples of 8; q (8, 8) -> the decoded plane: FDCT, quantise, dequantise, IDCT per 8 x 8 block."""
    h, w = p.shape
    blk = (p.astype(np.int64) - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)       # (by, bx, row, col)
    c = _fdct_pass(blk, True)                                                                   # along every row
    c = _fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)                                  # along every column
    q = np.asarray(q, dtype=np.int64).reshape(8, 8)
    q8 = 8 * q
    k = np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)
    c = k * q
    c = _idct_pass(c.swapaxes(-1, -2), True).swapaxes(-1, -2)                                   # columns first
    c = _range_limit(_idct_pass(c, False))
    return c.transpose(0, 2, 1, 3).reshape(h, w)


def _upsample(d):
    """h2v2 fancy upsample of a decoded (h, w) plane -> (2 h, 2 w)."""
    h, w = d.shape
    up, dn = d[np.maximum(np.arange(h) - 1, 0)], d[np.minimum(np.arange(h) + 1, h - 1)]
    s = np.empty((2 * h, w), dtype=np.int64)
    s[0::2], s[1::2] = 3 * d + up, 3 * d + dn
    left, right = s[:, np.maximum(np.arange(w) - 1, 0)], s[:, np.minimum(np.arange(w) + 1, w - 1)]
    out = np.empty((2 * h, 2 * w), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4            # at the edges s[x -+ 1] = s[x]: 4 s + 8, 4 s + 7
    return out


def jpeg_roundtrip(img, ql, qc):
    """(H, W, 3) uint8 with H and W multiples of 16, two 8 x 8 tables with entries in [1, 255] -> the decoded (H, W, 3) uint8."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W, _ = img.shape
    assert H % 16 == 0 and W % 16 == 0 and H > 0 and W > 0
    ql, qc = np.asarray(ql, dtype=np.int64).reshape(8, 8), np.asarray(qc, dtype=np.int64).reshape(8, 8)
    assert ql.min() >= 1 and ql.max() <= 255 and qc.min() >= 1 and qc.max() <= 255
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    bias = np.where(np.arange(W // 2) % 2 == 0, 1, 2)
    down = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
    y = _code_plane(y, ql)
    cb, cr = _upsample(_code_plane(down(cb), qc)) - 128, _upsample(_code_plane(down(cr), qc)) - 128
    out = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def jpeg_ref(img, quality):
    """(H, W, 3) uint8 -> Pillow's save(JPEG, quality) then open(), byte for byte; quality 0 is a copy (the table's `on == 0` row)."""
    if quality == 0:
        return np.ascontiguousarray(img, dtype=np.uint8).copy()
    return jpeg_roundtrip(img, *jpeg_quant_tables(quality))
