"""Pillow's `Image.transform(size, PERSPECTIVE, coeffs, BILINEAR, fillcolor=...)` on an RGB image, restated in numpy: the generic transform
of libImaging/Geometry.c with perspective_transform in place of affine_transform -- the source position is two fp64 quotients by one
denominator, every product and sum rounded on its own and evaluated left to right -- and from there on tests/affine_ref.py's sampling.
tests/test_perspective_cpu.py pins it against the installed Pillow bit for bit; the GPU tests compare the device kernel with Pillow itself
and use this file for the size, coefficient and policy lists and for what Pillow cannot give (the `inside` mask)."""
import numpy as np

from tests.affine_ref import FILL, PARAMS, SIZES as AFFINE_SIZES, affine_bilinear  # noqa: F401

SIZES = AFFINE_SIZES + [(5, 7)]                                                 # (H, W)
DISTORTIONS = [0.1, 0.3, 0.5, 0.9]
SEEDS = [0, 1, 2, 3, 4, 5]
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def positions(H, W, a):
    """(xin, yin) of every output pixel: den = a6 xc + a7 yc + 1, xin = (a0 xc + a1 yc + a2) / den, yin likewise."""
    a0, a1, a2, a3, a4, a5, a6, a7 = (np.float64(v) for v in a)
    xc = np.arange(W, dtype=np.float64)[None, :] + 0.5
    yc = np.arange(H, dtype=np.float64)[:, None] + 0.5
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den =a6 * xc + a7 * yc + 1.0
        return (a0 * xc + a1 * yc + a2) / den, (a3 * xc + a4 * yc + a5) / den, den


def perspective_bilinear(img, a, fill=FILL):
    """img: (H, W, 3) uint8; a: the eight coefficients (output pixel centre -> source position).  Returns (warped (H, W, 3) uint8,
    inside (H, W) bool = the pixels that were sampled, not filled).  A position that is infinite or NaN is outside."""
    H, W, _ = img.shape
    xin, yin, _ = positions(H, W, a)
    with np.errstate(invalid="ignore"):
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


def pil_perspective(img, a, fill=FILL):
    """The real thing."""
    from PIL import Image
    H, W, _ = img.shape
    return np.asarray(Image.fromarray(img).transform((W, H), Image.PERSPECTIVE, tuple(float(v) for v in a), Image.BILINEAR,
                                                     fillcolor=tuple(fill))).copy()


def policy_quad(W, H, D, seed):
    """The four output corners (tl, tr, br, bl) `TrainAugmentation.perspective_draws_for` makes from eight uniforms, here numpy's."""
    u = np.random.default_rng(1000 * seed + int(D * 100)).uniform(0, 1, 8).tolist()
    hw, hh = D * W / 2, D * H / 2
    return [(u[0] * hw, u[1] * hh), (W - u[2] * hw, u[3] * hh), (W - u[4] * hw, H - u[5] * hh), (u[6] * hw, H - u[7] * hh)]


def frame_quad(W, H):
    return [(0.0, 0.0), (float(W), 0.0), (float(W), float(H)), (0.0, float(H))]


def policy_coeffs(W, H, D, seed):
    """(inverse, forward) coefficients of one policy draw at size (W, H)."""
    from structuredetector_amd.data.augment import perspective_coeffs
    quad = policy_quad(W, H, D, seed)
    return perspective_coeffs(frame_quad(W, H), quad), perspective_coeffs(quad, frame_quad(W, H))


def affine_rows(W, H):
    """The pure-affine rows of tests/affine_ref.PARAMS at size (W, H), padded with a6 = a7 = 0."""
    from structuredetector_amd.data.augment import affine_inverse_matrix
    return [affine_inverse_matrix((W, H), a, s, (tx, ty)) + [0.0, 0.0] for a, s, tx, ty in PARAMS]


def hand_made(W, H):
    """Coefficient sets on which Pillow is well defined (no 0 / 0) and where the policy never lands:
    sign, sign2  a denominator that changes sign inside the frame;
    behind       numerators and denominator negative together right of x = 10: positions inside the source where den < 0, sampled;
    zero         a denominator that is exactly 0 at the pixel centre (1.5, 0.5) -- -0.5 * 1.5 + -0.5 * 0.5 + 1 in exact binary fractions --
                 with the numerators 4.5 and 3.5: an infinite position, fill."""
    return {"sign": (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.02, 0.001), "sign2": (0.9, 0.1, 1.0, -0.1, 0.9, 2.0, 0.004, -0.05),
            "behind": (-1.0, 0.0, 0.0, 0.0, -1.0, 0.0, -0.1, 0.0), "zero": (1.0, 0.0, 3.0, 0.0, 1.0, 3.0, -0.5, -0.5)}


def image(H, W, seed=0):
    img = np.random.default_rng(H * 1000 + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img
