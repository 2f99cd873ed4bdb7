"""The two histogram tone curves of `sd_tone_u8` restated in numpy -- ImageOps.equalize and ImageOps.autocontrast as closed forms over a
channel's histogram -- and Pillow itself as their oracle.  tests/test_tone_cpu.py pins `tone_ref` to Pillow byte for byte; the GPU tests
then compare the kernels with either.  A table row is [mode, cut_lo, cut_hi, 0]: mode 1 = autocontrast, 2 = equalize, anything else copies;
the cuts are clamped to [0, n]."""
import numpy as np

COPY, AUTOCONTRAST, EQUALIZE = 0, 1, 2
IDENTITY = np.arange(256, dtype=np.uint8)


def equalize_lut(h):
    """h: 256 counts -> the 256-entry table of ImageOps.equalize for that channel (32-bit unsigned arithmetic)."""
    h = np.asarray(h, dtype=np.int64)
    filled = np.flatnonzero(h)
    if len(filled) < 2:
        return IDENTITY.copy()
    step = (int(h.sum()) - int(h[filled[-1]])) // 255
    if step == 0:
        return IDENTITY.copy()
    below = np.concatenate([[0], np.cumsum(h)[:-1]])                 # h[0] + .. + h[i - 1]
    return np.minimum(255, (step // 2 + below) // step).astype(np.uint8)


def autocontrast_lo_hi(h, cut_lo, cut_hi):
    """(lo, hi) of ImageOps.autocontrast after its cuts, or None where it leaves the channel alone."""
    h = np.asarray(h, dtype=np.int64)
    n = int(h.sum())
    cut_lo, cut_hi = min(max(int(cut_lo), 0), n), min(max(int(cut_hi), 0), n)
    if cut_lo + cut_hi >= n:
        return None
    up = np.cumsum(h)                                                # h[0] + .. + h[i]
    down = np.cumsum(h[::-1])[::-1]                                  # h[i] + .. + h[255]
    lo = int(np.flatnonzero(up > cut_lo)[0])
    hi = int(np.flatnonzero(down > cut_hi)[-1])
    return (lo, hi) if hi > lo else None


def stretch_lut(lo, hi):
    """The table of ImageOps.autocontrast for hi > lo: IEEE double, the product and the sum rounded one after the other (numpy float64
    arithmetic does exactly that), truncated towards zero, clamped."""
    scale = np.float64(255.0) / np.float64(hi - lo)
    offset = np.float64(-lo) * scale
    t = np.arange(256, dtype=np.float64) * scale + offset
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def autocontrast_lut(h, cut_lo, cut_hi):
    pair = autocontrast_lo_hi(h, cut_lo, cut_hi)
    return IDENTITY.copy() if pair is None else stretch_lut(*pair)


def tone_ref(img, row):
    """img (H, W, 3) uint8, row [mode, cut_lo, cut_hi, ...] -> what `sd_tone_u8` must give for that image."""
    img = np.asarray(img)
    mode = int(row[0])
    if mode not in (AUTOCONTRAST, EQUALIZE):
        return img.copy()
    out = np.empty_like(img)
    for c in range(3):
        h = np.bincount(img[..., c].reshape(-1), minlength=256)
        lut = equalize_lut(h) if mode == EQUALIZE else autocontrast_lut(h, row[1], row[2])
        out[..., c] = lut[img[..., c]]
    return out


def cut_of(n_pixels, cutoff):
    """Pillow's own expression for the pixels autocontrast ignores at either end (cutoff a Python float or int)."""
    return int(n_pixels * cutoff // 100)


def pillow_tone(img, mode, cutoff=0):
    """Pillow itself: ImageOps.equalize(img) or ImageOps.autocontrast(img, cutoff) on an RGB image."""
    from PIL import Image, ImageOps
    im = Image.fromarray(np.ascontiguousarray(img), "RGB")
    if mode == EQUALIZE:
        im = ImageOps.equalize(im)
    elif mode == AUTOCONTRAST:
        im = ImageOps.autocontrast(im, cutoff=cutoff)
    return np.asarray(im).copy()


KINDS = ["noise", "constant", "two_valued", "narrow", "mostly_one"]


def tone_image(kind, h, w, rng):
    """The content kinds of the tests: uniform noise, one colour, two values, a narrow band, and 90 % one value (the last two and the
    constant frame are the histogram kernel's contention path)."""
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "constant":
        return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()
    if kind == "two_valued":
        pair = rng.integers(0, 256, (2, 3))
        return np.where(rng.integers(0, 2, (h, w, 1)) > 0, pair[0], pair[1]).astype(np.uint8)
    if kind == "narrow":
        base = rng.integers(0, 236, 3)
        return (base + rng.integers(0, 20, (h, w, 3))).astype(np.uint8)
    if kind == "mostly_one":
        noise = rng.integers(0, 256, (h, w, 3))
        return np.where(rng.random((h, w, 1)) < 0.9, rng.integers(0, 256, 3), noise).astype(np.uint8)
    raise ValueError(kind)
