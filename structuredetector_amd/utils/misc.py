"""Small host helpers kept for API parity with src/sdnet/utils/utils.py:324-338,364-381."""
from pathlib import Path

import numpy as np
import torch


def mkdir_if_needed(directory):
    Path(directory).mkdir(exist_ok=True)


def set_seed(seed=1975846251):
    torch.manual_seed(seed)
    np.random.seed(seed % (2**32))
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def clip_annotation(annotation, img_size):
    """utils.py:364-381: clamp every coordinate to [0, size-1], in place."""
    w, h = img_size
    cx = lambda v: min(max(v, 0), w - 1)
    cy = lambda v: min(max(v, 0), h - 1)
    for obj in annotation.objects:
        obj.x, obj.y = cx(obj.x), cy(obj.y)
        for p in obj.parts:
            p.x, p.y = cx(p.x), cy(p.y)
        if obj.box is not None:
            b = obj.box
            b.x_min, b.x_max, b.y_min, b.y_max = cx(b.x_min), cx(b.x_max), cy(b.y_min), cy(b.y_max)
    return annotation


def hflip_annotation(annotation, img_size):
    """utils.py:384-398: mirror every x about the image width, in place (boxes keep x_min <= x_max)."""
    w, _ = img_size
    for obj in annotation.objects:
        obj.x = w - obj.x - 1
        for p in obj.parts:
            p.x = w - p.x - 1
        if obj.box is not None:
            obj.box.x_min, obj.box.x_max = w - obj.box.x_max - 1, w - obj.box.x_min - 1
    return annotation


def vflip_annotation(annotation, img_size):
    """utils.py:401-415."""
    _, h = img_size
    for obj in annotation.objects:
        obj.y = h - obj.y - 1
        for p in obj.parts:
            p.y = h - p.y - 1
        if obj.box is not None:
            obj.box.y_min, obj.box.y_max = h - obj.box.y_max - 1, h - obj.box.y_min - 1
    return annotation


def transpose_annotation(annotation, img_size):
    """Follow a transpose of the image (x and y swapped), in place; img_size = (W, H) of the image BEFORE the transpose (the result lives in
    an H x W frame).  Every keypoint and box swaps its axes; nothing leaves the frame.  An involution, and transpose o hflip = vflip o
    transpose."""
    for obj in annotation.objects:
        obj.x, obj.y = obj.y, obj.x
        for p in obj.parts:
            p.x, p.y = p.y, p.x
        if obj.box is not None:
            b = obj.box
            b.x_min, b.x_max, b.y_min, b.y_max = b.y_min, b.y_max, b.x_min, b.x_max
    return annotation


def affine_annotation(annotation, forward_matrix, img_size):
    """Follow an affine warp of the image (data/augment.py: affine_forward_matrix), in place.  A pixel index p is the pixel centre p + 0.5
    -- the convention under which hflip_annotation's w - x - 1 holds -- so p' + 0.5 = F (p + 0.5); coordinates stay floats.  Unlike a flip, a
    warp can move points out of the frame, where clip_annotation would pin them to the border as false keypoints: they are dropped, by
    the warp's own inside test 0 <= x' + 0.5 < w and 0 <= y' + 0.5 < h.  An object whose anchor leaves goes with all its parts; a part that
    leaves is removed from its object; a box becomes the axis-aligned hull of its four corners (clip_annotation clips it later)."""
    w, h = img_size
    f0, f1, f2, f3, f4, f5 = forward_matrix

    def move(x, y):
        xc, yc = x + 0.5, y + 0.5
        return f0 * xc + f1 * yc + f2 - 0.5, f3 * xc + f4 * yc + f5 - 0.5

    def inside(x, y):
        return 0 <= x + 0.5 < w and 0 <= y + 0.5 < h

    kept = []
    for obj in annotation.objects:
        obj.x, obj.y = move(obj.x, obj.y)
        if not inside(obj.x, obj.y):
            continue
        parts = []
        for p in obj.parts:
            p.x, p.y = move(p.x, p.y)
            if inside(p.x, p.y):
                parts.append(p)
        obj.parts = parts
        if obj.box is not None:
            b = obj.box
            xs, ys = zip(*(move(x, y) for x in (b.x_min, b.x_max) for y in (b.y_min, b.y_max)))
            b.x_min, b.x_max, b.y_min, b.y_max = min(xs), max(xs), min(ys), max(ys)
        kept.append(obj)
    annotation.objects = kept
    return annotation


def perspective_annotation(annotation, forward8, img_size, affine_forward=None):
    """Follow a perspective warp of the image (data/augment.py: perspective_coeffs with the quads swapped), in place: with q = p + 0.5 a
    point moves to p' + 0.5 = ((f0 qx + f1 qy + f2) / den, (f3 qx + f4 qy + f5) / den), den = f6 qx + f7 qy + 1.  With `affine_forward`
    (affine_forward_matrix) the point goes through that matrix first, with nothing dropped in between: the image is warped once by the
    composed coefficients, so the inside test runs once, at the end.  The drop rule is affine_annotation's -- 0 <= x' + 0.5 < w and
    0 <= y' + 0.5 < h -- plus den > 0: a point with den <= 0 lies on or behind the horizon of the forward map, and where it would land is
    not where the image shows it.  An object whose anchor is dropped goes with all its parts; a dropped part is removed from its object; a
    box becomes the axis-aligned hull of its four corners, or the whole frame when a corner has den <= 0 (the quadrilateral is then
    unbounded; clip_annotation clips either later)."""
    w, h = img_size
    f0, f1, f2, f3, f4, f5, f6, f7 = forward8
    a = affine_forward

    def move(x, y):
        xc, yc = x + 0.5, y + 0.5
        if a is not None:
            xc, yc = a[0] * xc + a[1] * yc + a[2], a[3] * xc + a[4] * yc + a[5]
        den = f6 * xc + f7 * yc + 1.0
        if not den > 0:
            return None
        return (f0 * xc + f1 * yc + f2) / den - 0.5, (f3 * xc + f4 * yc + f5) / den - 0.5

    def inside(p):
        return p is not None and 0 <= p[0] + 0.5 < w and 0 <= p[1] + 0.5 < h

    kept = []
    for obj in annotation.objects:
        anchor = move(obj.x, obj.y)
        if not inside(anchor):
            continue
        obj.x, obj.y = anchor
        parts = []
        for p in obj.parts:
            moved = move(p.x, p.y)
            if inside(moved):
                p.x, p.y = moved
                parts.append(p)
        obj.parts = parts
        if obj.box is not None:
            b = obj.box
            corners = [move(x, y) for x in (b.x_min, b.x_max) for y in (b.y_min, b.y_max)]
            if any(c is None for c in corners):
                b.x_min, b.x_max, b.y_min, b.y_max = 0.0, float(w - 1), 0.0, float(h - 1)
            else:
                xs, ys = zip(*corners)
                b.x_min, b.x_max, b.y_min, b.y_max = min(xs), max(xs), min(ys), max(ys)
        kept.append(obj)
    annotation.objects = kept
    return annotation


def mosaic_annotation(annotation, sources, forward_matrices, rects):
    """Follow a mosaic of the image (data/augment.py: mosaic_tiles): `annotation` gets, in place, the objects of the four `sources` (the
    RESIZED annotations of the images shown in tiles 0 .. 3; they are read, never modified: every object is cloned first, so an image can
    be itself, its own partner and someone else's) moved by each tile's forward matrix, p' + 0.5 = F_q (p + 0.5) as in affine_annotation, and
    kept iff the point lies inside the tile's rectangle (x0, y0, x1, y1): x0 <= x' + 0.5 < x1 and y0 <= y' + 0.5 < y1 -- the pixels of the
    composite that tile owns.  An object whose anchor fails goes with all its parts; a failing part is removed from its object; a box
    becomes the hull of its corners (clip_annotation clips it later).  Objects are concatenated in tile order; image_path / img_size stay."""
    objects = []
    for source, (f0, f1, f2, f3, f4, f5), (x0, y0, x1, y1) in zip(sources, forward_matrices, rects):
        if x0 >= x1 or y0 >= y1:
            continue

        def move(x, y):
            xc, yc = x + 0.5, y + 0.5
            return f0 * xc + f1 * yc + f2 - 0.5, f3 * xc + f4 * yc + f5 - 0.5

        def inside(x, y):
            return x0 <= x + 0.5 < x1 and y0 <= y + 0.5 < y1

        for obj in source.objects:
            x, y = move(obj.x, obj.y)
            if not inside(x, y):
                continue
            obj = obj.clone()
            obj.x, obj.y = x, y
            parts = []
            for p in obj.parts:
                p.x, p.y = move(p.x, p.y)
                if inside(p.x, p.y):
                    parts.append(p)
            obj.parts = parts
            if obj.box is not None:
                b = obj.box
                xs, ys = zip(*(move(bx, by) for bx in (b.x_min, b.x_max) for by in (b.y_min, b.y_max)))
                b.x_min, b.x_max, b.y_min, b.y_max = min(xs), max(xs), min(ys), max(ys)
            objects.append(obj)
    annotation.objects = objects
    return annotation


def letterbox_geometry(in_size, out_size):
    """The aspect-preserving resize of `--keep_aspect`: a (win, hin) = in_size source in a (W, H) = out_size frame -> (wi, hi, px, py), the
    size of the resized image -- the largest of the source's aspect ratio that fits the frame, the free side rounded to the nearest
    integer -- and where its top-left corner is pasted (centred, the odd pixel of a bar after it).  Integer arithmetic only:
    width binds when W * hin <= H * win: wi = W, hi = min(H, max(1, (hin * W + win // 2) // win)); otherwise hi = H and wi likewise."""
    (win, hin), (W, H) = (int(v) for v in in_size), (int(v) for v in out_size)
    if min(win, hin, W, H) <= 0:
        raise ValueError(f"letterbox_geometry: sizes should be positive, not {win} x {hin} in {W} x {H}")
    if W * hin <= H * win:
        wi, hi = W, min(H, max(1, (hin * W + win // 2) // win))
    else:
        wi, hi = min(W, max(1, (win * H + hin // 2) // hin)), H
    return wi, hi, (W - wi) // 2, (H - hi) // 2


def shift_annotation(annotation, dx, dy):
    """Move every keypoint and box by (dx, dy), in place.  Nothing is dropped and nothing is clipped: a shift by (0, 0) leaves every
    coordinate bit for bit as it was."""
    for obj in annotation.objects:
        obj.x, obj.y = obj.x + dx, obj.y + dy
        for p in obj.parts:
            p.x, p.y = p.x + dx, p.y + dy
        if obj.box is not None:
            b = obj.box
            b.x_min, b.x_max, b.y_min, b.y_max = b.x_min + dx, b.x_max + dx, b.y_min + dy, b.y_max + dy
    return annotation


def letterbox_annotation(annotation, in_size, out_size):
    """Follow the letterbox of an image (in place): ORIGINAL pixels of a (win, hin) = in_size source -> pixels of the (W, H) = out_size
    frame: `resize` to the inner image, then the shift by its corner.  The inner image lies inside the frame, so nothing leaves it and
    nothing is dropped: `resize` is the plain scale x * wi / win (transforms.py:58), under which a point in the last source pixel lands
    up to a pixel past wi - 1 and is pinned by clip_annotation afterwards, exactly as on the stretched path -- with no bars (px = py = 0)
    the result is the stretched path's bit for bit."""
    wi, hi, px, py = letterbox_geometry(in_size, out_size)
    annotation.resize(tuple(in_size), (wi, hi))
    return shift_annotation(annotation, px, py)


def unletterbox_annotation(annotation, in_size, out_size):
    """The way back from `letterbox_annotation` (in place): pixels of the (W, H) = out_size frame -> ORIGINAL pixels of the (win, hin) =
    in_size source: the shift by (-px, -py), then `resize` (wi, hi) -> (win, hin).  Nothing is dropped: a prediction inside a bar lands
    outside the source, where the caller can see it."""
    wi, hi, px, py = letterbox_geometry(in_size, out_size)
    return shift_annotation(annotation, -px, -py).resize((wi, hi), tuple(in_size))


def get_unique_color_map(labels):
    """utils.py:476-479: a stable RGB triple per name (first three bytes of its xxh64 digest)."""
    from xxhash import xxh64_digest
    return {n: (*xxh64_digest(n.encode())[:3],) for n in labels}


def files_with_extension(folder, extension: str):
    """utils.py:327-328."""
    return [f for f in Path(folder).iterdir() if f.suffix == extension]


class AverageMeter:
    """Running mean of the values passed to `update` (reference: src/sdnet/utils/utils.py:311-324; same attributes `sum`, `count`, `avg`)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.sum, self.count, self.avg = 0.0, 0, 0.0

    def update(self, value):
        self.sum += value
        self.count += 1
        self.avg = self.sum / self.count
        return self.avg


def dict_grouping(iterable, key):
    """{key(element): [elements in input order]} (reference: src/sdnet/utils/utils.py:470-474; used by its Evaluator to split by label / kind)."""
    groups = {}
    for element in iterable:
        groups.setdefault(key(element), []).append(element)
    return groups

