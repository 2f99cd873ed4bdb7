"""Numpy restatement of Pillow's `Image.filter(ImageFilter.GaussianBlur(r))` on an RGB image (libImaging/BoxBlur.c: ImagingGaussianBlur
with three passes -> ImagingBoxBlur -> ImagingLineBoxBlur8), the reference the blur kernels are held to byte for byte.  It is pinned
against Pillow itself in tests/test_blur_cpu.py; the GPU tests compare `sd_blur_u8` with this file, never with the library's own host code.

GaussianBlur(r), r > 0 = three box-blur passes along every row, then the same three along every column; every pass rounds to bytes,
channels are independent, r == 0 is a copy.  The box radius is float32 arithmetic (`sqrt` and `floor` take doubles, as in C), the weights
are 24-bit fixed point, and the edge rule is replication of the pass's own input line.
"""
import math

import numpy as np

f32 = np.float32


def box_radius(r):
    """_gaussian_blur_radius: the (fractional) box radius whose three passes approximate a gaussian of standard deviation r."""
    r = f32(r)
    s2 = f32(f32(r * r) / f32(3))
    L = f32(math.sqrt(12.0 * float(s2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * s2)))
    a = f32(a / f32(f32(6) * f32(s2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    return f32(l + a)


def box_params(r):
    """(R, ww, fw) of ImagingLineBoxBlur8 for GaussianBlur(r): whole radius, 24-bit weight of a whole pixel, weight of the two edge pixels."""
    fr = box_radius(r)
    R = int(fr)
    ww = int(f32(1 << 24) / f32(fr * f32(2) + f32(1)))           # a float32 division, then truncation to uint32
    fw = ((1 << 24) - (R * 2 + 1) * ww) // 2
    return R, ww, fw


def box_pass(a, axis, R, ww, fw):
    """One pass along `axis` of a uint8 array: out[x] = (ww * sum_{-R..R} in[c(x+i)] + fw * (in[c(x-R-1)] + in[c(x+R+1)]) + 2^23) >> 24."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    n = a.shape[0]
    x = np.arange(n)
    c = lambda i: np.clip(i, 0, n - 1)
    acc = np.zeros_like(a)
    for i in range(-R, R + 1):
        acc += a[c(x + i)]
    out = (ww * acc + fw * (a[c(x - R - 1)] + a[c(x + R + 1)]) + (1 << 23)) >> 24
    assert out.min() >= 0 and out.max() <= 255
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def blur_params(a, R, ww, fw):
    """(H, W, 3) uint8 -> the six passes with given integer parameters (what one row of the device table asks for)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if R == 0 and fw == 0:
        return a.copy()
    for axis in (1, 0):                                          # rows first, then columns
        for _ in range(3):
            a = box_pass(a, axis, R, ww, fw)
    return a


def blur_ref(a, r):
    """(H, W, 3) uint8, radius r >= 0 -> Image.filter(GaussianBlur(r)) byte for byte."""
    if r == 0:
        return np.ascontiguousarray(a, dtype=np.uint8).copy()
    return blur_params(a, *box_params(r))
