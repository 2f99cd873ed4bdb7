"""The mosaic composite on the host, for tests/test_mosaic_cpu.py and tests/test_gpu_mosaic.py: image b's canvas is cut at (cx, cy) into
quadrants q = (x >= cx) + 2 (y >= cy), and quadrant q is `Image.transform((W, H), AFFINE, m_q, BILINEAR, fillcolor=FILL)` of resized image
s_q, read at the same pixel.  `pil_mosaic` builds it with Pillow itself (four transforms and a quadrant select), `numpy_mosaic` with
tests/affine_ref.py's restatement; `batch_tables` is the per-image table the GPU tests share."""
import numpy as np

from tests.affine_ref import FILL, affine_bilinear, pil_affine


def quadrants(H, W, cx, cy):
    """(H, W) int array of q = (x >= cx) + 2 (y >= cy)."""
    return (np.arange(W)[None, :] >= cx).astype(np.int64) + 2 * (np.arange(H)[:, None] >= cy)


def _compose(resized, geom, mats, transform):
    H, W, _ = resized[0].shape
    cx, cy, *src = geom
    q = quadrants(H, W, cx, cy)
    out = np.empty((H, W, 3), np.uint8)
    for k in range(4):
        if (q == k).any():
            out[q == k] = transform(resized[src[k]], mats[k])[q == k]
    return out


def pil_mosaic(resized, geom, mats):
    """resized: sequence of (H, W, 3) uint8 images of one size; geom = [cx, cy, s0, s1, s2, s3]; mats = four inverse matrices."""
    return _compose(resized, geom, mats, lambda im, m: pil_affine(im, m, FILL))


def numpy_mosaic(resized, geom, mats):
    return _compose(resized, geom, mats, lambda im, m: affine_bilinear(im, m, FILL)[0])


def clamped(geom, B, W, H):
    """The table row the kernels act on: centre clamped to [0, W] x [0, H], sources to [0, B)."""
    cx, cy, *src = geom
    return [min(max(cx, 0), W), min(max(cy, 0), H), *(min(max(s, 0), B - 1) for s in src)]


FLIPS = [0, 1, 2, 3, 1, 2]                                                      # one per row of batch_tables: all four codes occur


def batch_tables(size):
    """(geom rows, matrices) for B = 6 images at size = (W, H):
    0 a policy centre with cx % 4 != 0 and cy % 16 != 0 (a thread's four pixels and a block's rows straddle tiles), partners repeat and include 0
    1 centre (0, 0): tile 3 only
    2 not selected: a copy
    3 general matrices: zoom 0.37 with a rotation, anisotropic, and two policy tiles, around an off-centre cut
    4 a policy centre at the corner of its range, all partners the image itself
    5 cx = W: the two left tiles only."""
    from structuredetector_amd.data.augment import affine_inverse_matrix, mosaic_tiles
    W, H = size
    cx, cy = W // 2 + 3, H // 2 + 1
    assert cx % 4 and cy % 16
    rows = [mosaic_tiles(size, 0, (cx, cy, (3, 0, 3))), mosaic_tiles(size, 1, (0, 0, (2, 2, 5))), mosaic_tiles(size, 2, None),
            mosaic_tiles(size, 3, (W // 4 + 1, 3 * H // 4, (1, 4, 1))), mosaic_tiles(size, 4, (3 * W // 4, H // 4, (4, 4, 4))),
            mosaic_tiles(size, 5, (W, H // 2 + 1, (0, 2, 1)))]
    geom = [r[0] for r in rows]
    mats = [[list(m) for m in r[1]] for r in rows]
    mats[3][0] = affine_inverse_matrix(size, 10.0, 0.37, (3.0, -2.0))
    mats[3][3] = [1.7, 0.0, -5.0, 0.0, 0.6, 2.5]
    return geom, mats
