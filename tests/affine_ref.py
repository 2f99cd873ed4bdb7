"""Pillow's `Image.transform(size, AFFINE, matrix, BILINEAR, fillcolor=...)` on an RGB image, restated in numpy: the generic transform of
libImaging/Geometry.c (affine_transform + bilinear_filter32RGB) in plain double arithmetic, every product and sum rounded on its own and
evaluated left to right, the result truncated to a byte.  tests/test_affine_cpu.py pins it against the installed Pillow bit for bit; the
GPU tests compare the device kernels with Pillow itself and use this file for what Pillow cannot give (expected positions, small images)."""
import numpy as np

SIZES = [(96, 128), (64, 64), (160, 96), (33, 47)]                              # (H, W)
PARAMS = [(0, 1, 0, 0), (17.3, 1.1, 3.25, -4.5), (-45, 0.75, 0, 0), (90, 1, 0, 0), (180, 1.25, -7, 2), (5, 0.9, 10.5, 10.5),
          (-133.7, 1.2, 0.3, 0.1)]                                              # (angle, scale, tx, ty)
FILL = (124, 116, 104)


def affine_bilinear(img, m, fill=FILL):
    """img: (H, W, 3) uint8; m: the six coefficients of the inverse matrix (output pixel centre -> source position).
    Returns (warped (H, W, 3) uint8, inside (H, W) bool = the pixels that were sampled, not filled)."""
    H, W, _ = img.shape
    m0, m1, m2, m3, m4, m5 = (np.float64(v) for v in m)
    xc = np.arange(W, dtype=np.float64)[None, :] + 0.5
    yc = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xin = m0 * xc + m1 * yc + m2
    yin = m3 * xc + m4 * yc + m5
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    xin = np.where(inside, xin, 0.5) - 0.5
    yin = np.where(inside, yin, 0.5) - 0.5
    X = np.floor(xin).astype(np.int64)
    Y = np.floor(yin).astype(np.int64)
    dx = (xin - X)[..., None]
    dy = (yin - Y)[..., None]
    x0, x1, yc0 = np.clip(X, 0, W - 1), np.clip(X + 1, 0, W - 1), np.clip(Y, 0, H - 1)
    p = img.astype(np.float64)
    v1 = p[yc0, x0] + (p[yc0, x1] - p[yc0, x0]) * dx
    has_row = (Y + 1 >= 0) & (Y + 1 < H)
    y1 = np.where(has_row, Y + 1, yc0)
    v2 = np.where(has_row[..., None], p[y1, x0] + (p[y1, x1] - p[y1, x0]) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.uint8)                                # truncation, like the C cast
    out[~inside] = np.asarray(fill, np.uint8)
    return out, inside


def pil_affine(img, m, fill=FILL):
    """The real thing: what torchvision's F.affine calls for a PIL image."""
    from PIL import Image
    H, W, _ = img.shape
    return np.asarray(Image.fromarray(img).transform((W, H), Image.AFFINE, tuple(m), Image.BILINEAR, fillcolor=tuple(fill))).copy()


def blob_image(H, W, points, value=255):
    """A black (H, W, 3) image with a 3 x 3 block of `value` centred on every (x, y) of points (integer pixel indices)."""
    img = np.zeros((H, W, 3), np.uint8)
    for x, y in points:
        img[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = value
    return img
