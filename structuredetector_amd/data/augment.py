"""GPU input pipeline: the reference's per-sample PIL / torchvision chain
`Resize -> [ColorJitter] -> RandomHorizontalFlip -> RandomVerticalFlip -> Normalize` (src/sdnet/data/transforms.py:217-234,
validation :255-261) for a whole batch in two HIP launches (`sd_preprocess_images`), with the annotation transforms of
src/sdnet/utils/utils.py:384-415 on the host and the per-epoch multi-scale shapes of transforms.py:237-244.

Resize parity: `F.resize` of a PIL image is Pillow's separable 8-bit fixed-point resampling; `pil_bilinear_coeffs` reproduces
Pillow's coefficient tables (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc) and the kernels its integer
arithmetic, so the resized bytes equal `Image.resize(size, BILINEAR)` and the normalised tensor equals the reference's bit for bit.
ColorJitter parity (transforms.py:37-47): torchvision's ColorJitter on a PIL image is Pillow's ImageEnhance.Brightness / Contrast /
Color plus an HSV round trip for the hue, in a random order; `sd_preprocess_images_jitter` reproduces Pillow's byte arithmetic on the
resized image (oracle/pil_photometric.py is the restatement, pinned against Pillow over all 2^24 colours; torchvision itself is absent
here, its PIL code path is restated from the published 0.20.1 source), so with the same random draws the normalised tensor equals the
reference's bit for bit.  The random draws come from torch's global generator on the host (TrainAugmentation.draws_for).
Random affine (`--aug_rotate / --aug_scale / --aug_translate`; not in the reference): where torchvision's RandomAffine would sit, between
Resize and ColorJitter, as Pillow's `Image.transform(size, AFFINE, matrix, BILINEAR, fillcolor=_FILL)` byte for byte
(`sd_preprocess_images_affine`); the matrices are built on the host (`affine_inverse_matrix`), the annotations follow with
`utils.misc.affine_annotation`, which drops what leaves the frame.
Mosaic (`--aug_mosaic P`; not in the reference): between Resize and the warp, a selected image becomes four images of its size group at
half scale around a random centre (`mosaic_tiles`), each quadrant Pillow's `Image.transform` of its source byte for byte
(`sd_preprocess_images_mosaic`); `utils.misc.mosaic_annotation` gathers the four annotations and keeps what each tile shows.
Window (`--train_tiles CxR`; not in the reference): the Resize itself targets the canvas tiled inference shows the network (`tile_canvas`) and
only a W x H window of it at a random origin is produced, `Image.resize(canvas, BILINEAR).crop(window)` byte for byte
(`sd_preprocess_images_window`: the source rows and columns under the window are all that is read); every later stage works on the window,
the annotations follow with `ann.resize` to the canvas and `affine_annotation` by the shift.
Letterbox (`--keep_aspect`; not in the reference): the Resize keeps the source's aspect ratio -- the largest wi x hi that fits W x H
(`letterbox_geometry`, integers only) -- and the resized image sits centred in a W x H frame of `_FILL`, byte for byte
`Image.new("RGB", (W, H), _FILL).paste(Image.resize((wi, hi), BILINEAR), (px, py))` (`sd_preprocess_images_letterbox`: the plain horizontal
pass at width wi, then one vertical pass that writes image and bars); every later stage works on the frame, the annotations follow with
`ann.resize` to the inner image and a shift by (px, py) that drops nothing (`utils.misc.letterbox_annotation`'s rule);
`utils.misc.unletterbox_annotation` is the way back.
Blur (`--aug_blur R`; not in the reference): between the warp and the ColorJitter, a selected image is `Image.filter(GaussianBlur(r))`
byte for byte -- Pillow's six rounded box-blur passes in integer arithmetic (`sd_blur_u8`; in the chain `sd_preprocess_images_blur`); the
box radius and weights of a pass are float32 arithmetic restated on the host (`blur_box_params`).  Photometric: annotations are untouched.
Perspective (`--aug_perspective D`; not in the reference): the warp slot of the chain becomes one homography, the random affine folded into
it on the host (`compose_affine_perspective`), byte for byte `Image.transform(size, PERSPECTIVE, coeffs, BILINEAR, fillcolor)`
(`sd_perspective_u8`; in the chain `sd_preprocess_images_persp`); the annotations follow with `utils.misc.perspective_annotation`.
JPEG (`--aug_jpeg QMIN`; not in the reference): between the blur and the ColorJitter, a selected image is what Pillow's
`save(buf, "JPEG", quality=q)` then `open(buf)` gives, byte for byte -- colour conversion, 4:2:0 chroma, the accurate-integer DCT of every
8 x 8 block, the quantiser and the way back, all integer (`sd_jpeg_u8`; in the chain `sd_preprocess_images_jpeg`); the two quantisation
tables of a quality come from the host (`jpeg_quant_tables`).  Photometric: annotations are untouched.
Noise (`--aug_noise R` / `--aug_noise_shot G`; not in the reference): between the blur and the JPEG round trip -- optics, sensor, encoder --
a selected image gets read noise of a standard deviation up to R grey levels plus shot noise whose variance is up to G levels^2 per level:
the heteroscedastic-Gaussian sensor model per channel and pixel in the 8-bit domain (no gamma is modelled), all integer and bit-exact
(`sd_noise_u8`; in the chain `sd_preprocess_images_noise`; tests/noise_ref.py restates it).  The random numbers are made on the device by a
counter-based generator, Philox4x32-10 keyed per image and counted by the byte's offset in its image, so the bytes depend on the image and
its row (`noise_rows`) alone; the host draws only the two key words and the two strengths.  Photometric: annotations are untouched.
Tone (`--aug_equalize P` / `--aug_autocontrast P`; not in the reference): after the JPEG round trip, in front of the ColorJitter, a selected
image is Pillow's `ImageOps.equalize(img)` or `ImageOps.autocontrast(img, cutoff)`, byte for byte -- a look-up table per channel made from
the histogram of the 8-bit frame as it stands there, fill colour and letterbox bars included (`sd_tone_u8`; in the chain
`sd_preprocess_images_tone`); the host only turns the cutoff into pixel counts (`tone_rows`).  Photometric: annotations are untouched.
Transpose (`--aug_transpose P`; not in the reference): last, after the flips, a selected image of the assembled (square) batch has its x and
y swapped (`sd_transpose_select`, one launch: lossless, with the flips the eight symmetries of the grid); the annotations follow with
`utils.misc.transpose_annotation`.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from .. import _lib as L
from ..utils.args import AUG_FLAGS, aug_flag, parse_tiles, tile_canvas
from ..utils.misc import (affine_annotation, clip_annotation, hflip_annotation, letterbox_annotation, letterbox_geometry, mosaic_annotation,
                          perspective_annotation, transpose_annotation, vflip_annotation)

PRECISION_BITS = 32 - 8 - 2
_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)
_FILL = (124, 116, 104)          # what the affine warp leaves uncovered: the ImageNet mean in bytes (about 0 after Normalize)


def pil_bilinear_coeffs(in_size: int, out_size: int):
    """Pillow's precompute_coeffs (triangle filter, support 1.0 scaled by max(in/out, 1)) + normalize_coeffs_8bpc for one axis.
    Returns (bounds int32 (out, 2) = first source index and tap count, kk int32 (out, ksize) 22-bit fixed-point weights, ksize).
    Plain Python floats are C doubles and int() truncates like a C cast, so every intermediate matches Pillow's."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        ww = 0.0
        k = []
        for x in range(xmax):
            a = (x + xmin - center + 0.5) * ss
            if a < 0.0:
                a = -a
            w = 1.0 - a if a < 1.0 else 0.0
            k.append(w)
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
            v = k[x] * (1 << PRECISION_BITS)
            kk[xx, x] = int(-0.5 + v) if k[x] < 0 else int(0.5 + v)
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


class _Tables:
    """Coefficient tables, one entry per (in_size, out_size) pair seen (a handful per run): the host copy, the device-resident copy, and
    the window extents read off the host copy."""

    def __init__(self):
        self.cache = {}
        self.host_cache = {}
        self.extents = {}

    def host(self, in_size, out_size):
        t = self.host_cache.get((in_size, out_size))
        if t is None:
            t = self.host_cache[(in_size, out_size)] = pil_bilinear_coeffs(in_size, out_size)
        return t

    def get(self, in_size, out_size, device):
        key = (in_size, out_size, device.index)
        t = self.cache.get(key)
        if t is None:
            bounds, kk, ksize = self.host(in_size, out_size)
            t = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize)
            self.cache[key] = t
        return t

    def extent(self, in_size, canvas_size, out_size):
        key = (in_size, canvas_size, out_size)
        e = self.extents.get(key)
        if e is None:
            bounds = self.host(in_size, canvas_size)[0]
            first, end = bounds[:, 0].tolist(), bounds.sum(1).tolist()                  # first source index, one past the last
            e = self.extents[key] = max(end[o + out_size - 1] - first[o] for o in range(canvas_size - out_size + 1))
        return e


_tables = _Tables()


def window_extents(in_size: int, canvas_size: int, out_size: int) -> int:
    """The largest source span, along one axis, of any `out_size` window of a resize in_size -> canvas_size: the maximum over the origins
    o in [0, canvas_size - out_size] of bounds[o + out_size - 1].first + count - bounds[o].first on `pil_bilinear_coeffs`' table.  What
    `sd_preprocess_images_window` takes as max_cols (width axis) and max_rows (height axis); cached with the tables."""
    in_size, canvas_size, out_size = int(in_size), int(canvas_size), int(out_size)
    if not 0 < out_size <= canvas_size:
        raise ValueError(f"a window of {out_size} does not fit a canvas of {canvas_size}")
    return _tables.extent(in_size, canvas_size, out_size)


def affine_inverse_matrix(size, angle, scale, translate):
    """torchvision's `_get_inverse_affine_matrix` with shear 0 about the image centre, in plain Python floats (C doubles): the six
    coefficients Pillow's `Image.transform(size, AFFINE, m, ...)` takes, mapping an OUTPUT pixel centre to its source position.
    size = (width, height), angle in degrees, translate = (tx, ty) in pixels.  Angle 0, scale 1, no shift: exactly [1, 0, 0, 0, 1, 0]."""
    w, h = size
    tx, ty = translate
    rot = math.radians(angle)
    cx, cy = w * 0.5, h * 0.5
    a, b, c, d = math.cos(rot), -math.sin(rot), math.sin(rot), math.cos(rot)
    m = [d / scale, -b / scale, 0.0, -c / scale, a / scale, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def affine_forward_matrix(size, angle, scale, translate):
    """The forward twin of `affine_inverse_matrix` (source position -> output position, both as pixel centres): what the annotations
    follow (`affine_annotation`).  out = scale * R(angle) * (in - centre) + centre + translate."""
    w, h = size
    tx, ty = translate
    rot = math.radians(angle)
    cx, cy = w * 0.5, h * 0.5
    a, b, c, d = scale * math.cos(rot), -scale * math.sin(rot), scale * math.sin(rot), scale * math.cos(rot)
    return [a, b, cx + tx - (a * cx + b * cy), c, d, cy + ty - (c * cx + d * cy)]


def perspective_coeffs(src_quad, dst_quad):
    """The 8 coefficients a0 .. a7 of the homography that takes the four `dst_quad` points to the four `src_quad` points,
    src = ((a0 x + a1 y + a2) / den, (a3 x + a4 y + a5) / den) with den = a6 x + a7 y + 1 at dst = (x, y): what Pillow's
    `Image.transform(size, PERSPECTIVE, coeffs, ...)` takes when dst are positions in the output and src in the source (both in the
    continuous frame, a pixel index p being p + 0.5).  An 8 x 8 `numpy.linalg.solve` in float64, not torchvision's float32 least squares.
    With the quads swapped it gives the forward twin, what the annotations follow (`perspective_annotation`)."""
    a = np.zeros((8, 8), np.float64)
    b = np.zeros(8, np.float64)
    for k, ((sx, sy), (dx, dy)) in enumerate(zip(src_quad, dst_quad)):
        a[2 * k] = (dx, dy, 1.0, 0.0, 0.0, 0.0, -dx * sx, -dy * sx)
        a[2 * k + 1] = (0.0, 0.0, 0.0, dx, dy, 1.0, -dx * sy, -dy * sy)
        b[2 * k], b[2 * k + 1] = sx, sy
    return np.linalg.solve(a, b).tolist()


def compose_affine_perspective(affine_inverse6, persp_inverse8):
    """The 8 coefficients of source = A_inv(P_inv(out)): the image is affine-warped first and perspective-warped second, in ONE resample.
    The 3 x 3 product of A_inv, extended by the row (0, 0, 1), with P_inv; its last row is P_inv's (a6, a7, 1), so nothing is
    renormalised.  With the identity perspective the result is the affine row padded with (0, 0), with the identity affine it is the
    perspective row, both exactly."""
    a0, a1, a2, a3, a4, a5 = (float(v) for v in affine_inverse6)
    p = [float(v) for v in persp_inverse8]
    return [a0 * p[0] + a1 * p[3] + a2 * p[6], a0 * p[1] + a1 * p[4] + a2 * p[7], a0 * p[2] + a1 * p[5] + a2,
            a3 * p[0] + a4 * p[3] + a5 * p[6], a3 * p[1] + a4 * p[4] + a5 * p[7], a3 * p[2] + a4 * p[5] + a5, p[6], p[7]]


def mosaic_tiles(size, i, draw):
    """One image's mosaic from (W, H) = size and draw = (cx, cy, (p1, p2, p3)) -- an integer centre and the three partner images -- or
    draw = None for an image that is not selected.  Returns (geom, inverse, forward, rects):
    geom    [cx, cy, s0, s1, s2, s3], the row of `sd_preprocess_images_mosaic`'s mosaic_geom: tile q = (x >= cx) + 2 (y >= cy) shows image s_q, s0 = i;
    inverse the four matrices m_q (canvas pixel centre -> source position) of its mosaic_affine;
    forward their twins (source -> canvas), what `mosaic_annotation` moves the points by;
    rects   (x0, y0, x1, y1) per tile: the canvas pixels x0 <= x < x1, y0 <= y < y1 that show the tile's source.
    Policy: every source at zoom 1/2 with a corner on the centre, so tile q's half image has its origin at ox = cx - W/2 (q = 0, 2) or cx
    (q = 1, 3), oy likewise with cy and H/2, m_q = [2, 0, -2 ox, 0, 2, -2 oy] (exact in double; every tap is a 2 x 2 block mean) and its
    rectangle is the half image cropped by the quadrant and the canvas; what the half image leaves of its quadrant is fill.  Not
    selected: the centre (W, H) makes tile 0 the whole canvas and the identity copies image i."""
    W, H = size
    if draw is None:
        ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        return [W, H, i, i, i, i], [list(ident) for _ in range(4)], [list(ident) for _ in range(4)], [(0, 0, W, H), (W, 0, W, H), (0, H, W, H), (W, H, W, H)]
    cx, cy, partners = draw
    inverse, forward, rects = [], [], []
    for q in range(4):
        ox = cx - W // 2 if q in (0, 2) else cx
        oy = cy - H // 2 if q < 2 else cy
        inverse.append([2.0, 0.0, -2.0 * ox, 0.0, 2.0, -2.0 * oy])
        forward.append([0.5, 0.0, float(ox), 0.0, 0.5, float(oy)])
        x0, x1 = (max(ox, 0), cx) if q in (0, 2) else (cx, min(ox + W // 2, W))
        y0, y1 = (max(oy, 0), cy) if q < 2 else (cy, min(oy + H // 2, H))
        rects.append((x0, y0, x1, y1))
    return [cx, cy, i, *partners], inverse, forward, rects


# field of the chain's descriptor: (numpy dtype path, row width, message) of its per-image host table.  The integer tables of the late stages
# go through int64 first, so a value past 2^31 wraps to the int32 bit pattern the library reads as uint32 instead of being refused.
_I32, _WRAP32, _F64 = (np.int32,), (np.int64, np.int32), (np.float64,)
_UPLOADS = {
    "flips": ((np.uint8,), 1, "flips must have one entry per image"),
    "jitter_order": (_I32, 1, "jitter parameters must have one row per image"),
    "jitter_factors": ((np.float32,), 3, "jitter parameters must have one row per image"),
    "mosaic_geom": (_I32, 6, "mosaic must have one geometry row of 6 integers and four matrices of 6 coefficients per image"),
    "mosaic_affine": (_F64, 24, "mosaic must have one geometry row of 6 integers and four matrices of 6 coefficients per image"),
    "window": (_I32, 2, "window must have one origin (x0, y0) per image"),
    "affine": (_F64, 6, "affine must have one row of 6 coefficients per image"),
    "persp": (_F64, 8, "persp must have one row of 8 coefficients per image"),
    "blur": (_WRAP32, 3, "blur must have one row (R, ww, fw) per image"),
    "noise": (_WRAP32, 4, "noise must have one row (k0, k1, a, b) per image"),
    "jpeg": (_WRAP32, 129, "jpeg must have one row (on, ql[64], qc[64]) per image"),
    "tone": (_WRAP32, 4, "tone must have one row (mode, cut_lo, cut_hi, 0) per image"),
}


def _upload(field, rows, B, device):
    """The host table `rows` of `field` (_UPLOADS) as a contiguous device tensor of B rows."""
    path, width, message = _UPLOADS[field]
    table = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows, dtype=path[0])
    for dtype in path[1:]:
        table = table.astype(dtype)
    table = torch.as_tensor(np.ascontiguousarray(table.reshape(-1, width) if width > 1 else table.reshape(-1)))
    if table.shape[0] != B:
        raise L.SdError(message)
    return table.to(device, non_blocking=True)


def _run_stage(name, images, rows, field=None, workspace=None, extra=()):
    """The shared body of the stand-alone stages `<name>_images`: images (B, H, W, 3) uint8 on the GPU and the B rows of the chain's table
    `field` (default: name) -> a new tensor from `sd_<name>_u8`, called with `extra` behind the table and, when workspace(lib, B, H, W)
    gives a size, that workspace."""
    L.require_cuda(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise L.SdError(f"{name}_images expects (B, H, W, 3) uint8, got {tuple(images.shape)} {images.dtype}")
    images = images.contiguous()
    B, H, W, _ = images.shape
    table = _upload(field or name, rows, B, images.device)
    out = torch.empty_like(images)
    lib = L.lib()
    if workspace is not None:
        ws = L.workspace(workspace(lib, B, H, W), images.device)
        extra = (*extra, ws.data_ptr(), ws.numel())
    L.check(getattr(lib, f"sd_{name}_u8")(images.data_ptr(), out.data_ptr(), B, H, W, table.data_ptr(), *extra, L.stream()), f"sd_{name}_u8")
    return out


def perspective_images(images: torch.Tensor, persp, fill=_FILL) -> torch.Tensor:
    """images: (B, H, W, 3) uint8 on the GPU; persp: B rows of 8 coefficients as `perspective_coeffs` makes them.  Returns a new tensor,
    image b = `Image.transform((W, H), PERSPECTIVE, persp_b, BILINEAR, fillcolor=fill)` byte for byte (`sd_perspective_u8`: the stand-alone
    stage of the chain)."""
    return _run_stage("perspective", images, persp, field="persp", extra=((C.c_ubyte * 3)(*fill),))


def blur_box_params(r):
    """(R, ww, fw) of Pillow's `GaussianBlur(r)` (libImaging/BoxBlur.c: _gaussian_blur_radius, ImagingLineBoxBlur8): the whole box radius
    and the 24-bit weights of a whole pixel and of the two edge pixels of one pass, one row of `sd_blur_u8`'s table.  Pillow computes them in
    float32 -- every operation below rounds to float32, only `sqrt` and `floor` take doubles as in C -- and the weight of a whole pixel is a
    float32 division truncated to uint32; double arithmetic changes bytes (r = 0.3, 0.7, 1.0).  r = 0 gives (0, 2^24, 0): a copy."""
    f = np.float32
    r = f(r)
    if not 0 <= r <= 8:
        raise ValueError(f"blur radius should be in [0, 8], not {r}")
    s2 = f(f(r * r) / f(3))
    ll = f(math.sqrt(12.0 * float(s2) + 1.0))
    l = f(math.floor((float(ll) - 1.0) / 2.0))
    a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * s2)))
    a = f(a / f(f(6) * f(s2 - f(f(l + f(1)) * f(l + f(1))))))
    fr = f(l + a)
    R = int(fr)
    ww = int(f(1 << 24) / f(fr * f(2) + f(1)))
    return R, ww, ((1 << 24) - (2 * R + 1) * ww) // 2


def blur_images(images: torch.Tensor, blur) -> torch.Tensor:
    """images: (B, H, W, 3) uint8 on the GPU; blur: B rows (R, ww, fw) as `blur_box_params` makes them.  Returns a new tensor, image b =
    `Image.filter(ImageFilter.GaussianBlur(r_b))` byte for byte (`sd_blur_u8`: the stand-alone stage of the chain)."""
    return _run_stage("blur", images, blur, workspace=lambda lib, B, H, W: lib.sd_blur_workspace_bytes(B, H, W))


# Annex K of the JPEG standard: the luminance and chrominance quantisation tables of quality 50, natural (row-major) order
_JPEG_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_JPEG_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def jpeg_quant_tables(q):
    """(ql, qc) of libjpeg's `jpeg_set_quality(q, force_baseline)`, what Pillow's `save(quality=q)` writes and `Image.open().quantization`
    returns: two lists of 64 entries in [1, 255] in natural (row-major) order, the Annex-K tables scaled by 5000 // q percent below quality 50
    and by 200 - 2 q from there on."""
    q = int(q)
    if not 1 <= q <= 100:
        raise ValueError(f"jpeg quality should be in [1, 100], not {q}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((v * s + 50) // 100, 1), 255) for v in base] for base in (_JPEG_LUMA, _JPEG_CHROMA))


def jpeg_rows(qualities):
    """One row [on, ql[64], qc[64]] of `sd_jpeg_u8`'s table per quality; quality 0 gives a copy row (on = 0, the tables all ones)."""
    rows = []
    for q in qualities:
        if int(q) == 0:
            rows.append([0] + [1] * 128)
        else:
            ql, qc = jpeg_quant_tables(q)
            rows.append([1, *ql, *qc])
    return rows


def jpeg_images(images: torch.Tensor, rows) -> torch.Tensor:
    """images: (B, H, W, 3) uint8 on the GPU with H and W multiples of 16; rows: B rows [on, ql[64], qc[64]] as `jpeg_rows` makes them.
    Returns a new tensor, image b = Pillow's `save(buf, "JPEG", quality=q_b)` then `open(buf)` byte for byte (`sd_jpeg_u8`: the stand-alone
    stage of the chain)."""
    return _run_stage("jpeg", images, rows, workspace=lambda lib, B, H, W: lib.sd_jpeg_workspace_bytes(B, H, W))


TONE_COPY, TONE_AUTOCONTRAST, TONE_EQUALIZE = 0, 1, 2               # the modes of `sd_tone_u8`'s table
TONE_STRIP_PIXELS = 16384                                            # include/sdnet_hip.h SD_TONE_STRIP_PIXELS: pixels of a histogram block


def tone_rows(draws, n_pixels):
    """One row [mode, cut_lo, cut_hi, 0] of `sd_tone_u8`'s table per draw (mode, cutoff percent) on images of n_pixels pixels: the two cuts
    are Pillow's `int(n * cutoff // 100)` with the cutoff a Python float, the number of darkest and of brightest pixels that
    `ImageOps.autocontrast(img, cutoff)` ignores; 0 for the other modes."""
    rows = []
    for mode, cutoff in draws:
        cut = int(int(n_pixels) * float(cutoff) // 100) if int(mode) == TONE_AUTOCONTRAST else 0
        rows.append([int(mode), cut, cut, 0])
    return rows


def tone_images(images: torch.Tensor, rows) -> torch.Tensor:
    """images: (B, H, W, 3) uint8 on the GPU, any H and W; rows: B rows [mode, cut_lo, cut_hi, 0] as `tone_rows` makes them.  Returns a
    new tensor, image b = Pillow's `ImageOps.autocontrast` (mode 1) or `ImageOps.equalize` (mode 2) of image b byte for byte, or image b
    itself (`sd_tone_u8`: the stand-alone stage of the chain)."""
    return _run_stage("tone", images, rows, workspace=lambda lib, B, H, W: lib.sd_tone_workspace_bytes(B))


def noise_rows(draws):
    """One row [k0, k1, a, b] of `sd_noise_u8`'s table per draw (k0, k1, sigma_read, gain): the two Philox key words, the read-noise
    variance a = round(sigma_read^2 65536) and the shot gain b = round(gain 65536), both Q16, all four as int32 bit patterns (the library
    reads them as uint32 and clamps a to 2^26, b to 2^17)."""
    wrap = lambda v: ((int(v) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000
    return [[wrap(k0), wrap(k1), wrap(round(float(sigma) * float(sigma) * 65536.0)), wrap(round(float(gain) * 65536.0))]
            for k0, k1, sigma, gain in draws]


def noise_images(images: torch.Tensor, rows) -> torch.Tensor:
    """images: (B, H, W, 3) uint8 on the GPU, any H and W; rows: B rows [k0, k1, a, b] as `noise_rows` makes them.  Returns a new tensor,
    image b = image b with the sensor noise of its row, byte for byte tests/noise_ref.py's `noise_ref`, or image b itself for a row with
    a = b = 0 (`sd_noise_u8`: the stand-alone stage of the chain)."""
    return _run_stage("noise", images, rows)


JPEG_MAX_QUALITY = 95                                                # the upper end of `--aug_jpeg`'s quality range (Pillow's advised maximum)
GEOM_STRETCH, GEOM_WINDOW, GEOM_LETTERBOX = 0, 1, 2                  # include/sdnet_hip.h SD_GEOM_*


def _chain_desc(source, is_list, B, Hin, Win, out_size, flips, mean, std, jitter, affine, mosaic, window, letterbox, blur, persp, jpeg, tone,
                noise, dev):
    """The descriptor of one `sd_preprocess_chain` call (include/sdnet_hip.h sd_preprocess_desc): source = the address of the packed images
    or, with is_list, of the pointer table; every other argument as `preprocess_images` takes it.  Each optional table is uploaded once,
    the geometry (coefficient tables, `window_extents`, the letterbox tuple) resolved once.  Returns (descriptor, out, the device tensors
    the descriptor points into)."""
    if persp is not None and affine is not None:
        raise L.SdError("preprocess: persp and affine do not combine (fold the affine matrix in with compose_affine_perspective)")
    if letterbox is not None and window is not None:
        raise L.SdError("preprocess: a letterbox and a window do not combine")
    Wout, Hout = int(out_size[0]), int(out_size[1])
    d = L.PreprocessDesc(images=source, list=int(is_list), geometry=GEOM_STRETCH, B=B, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout)
    Wt, Ht, org = Wout, Hout, None                                   # the resize target of the coefficient tables
    if letterbox is not None:
        wi, hi, px, py = (int(v) for v in letterbox)
        if wi <= 0 or hi <= 0:
            raise L.SdError(f"letterbox: the inner image should be at least 1 x 1, not {wi} x {hi}")
        d.geometry, d.Hg, d.Wg, d.g0, d.g1 = GEOM_LETTERBOX, hi, wi, py, px      # (the library checks that the image lies inside the frame)
        Wt, Ht = wi, hi
    elif window is not None:
        (Wc, Hc), origins = window
        Wt, Ht = int(Wc), int(Hc)
        if not (0 < Wout <= Wt and 0 < Hout <= Ht):
            raise L.SdError(f"window: {Wout} x {Hout} does not fit the canvas {Wt} x {Ht}")
        org = _upload("window", origins, B, dev)
        d.geometry, d.Hg, d.Wg, d.window = GEOM_WINDOW, Ht, Wt, org.data_ptr()
        d.g0, d.g1 = window_extents(Hin, Ht, Hout), window_extents(Win, Wt, Wout)   # (the LDS limit of the list form binds g1, the column span)
    hb, hk, d.h_ksize = _tables.get(Win, Wt, dev)
    vb, vk, d.v_ksize = _tables.get(Hin, Ht, dev)
    d.h_bounds, d.h_kk, d.v_bounds, d.v_kk = hb.data_ptr(), hk.data_ptr(), vb.data_ptr(), vk.data_ptr()
    out = torch.empty((B, 3, Hout, Wout), dtype=torch.float32, device=dev)
    d.out, d.fill3, d.mean3, d.std3 = out.data_ptr(), (C.c_ubyte * 3)(*_FILL), (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    keep = [org, hb, hk, vb, vk]

    given = dict(flips=flips, jitter_order=jitter and jitter[0], jitter_factors=jitter and jitter[1], mosaic_geom=mosaic and mosaic[0],
                 mosaic_affine=mosaic and mosaic[1], affine=affine, persp=persp, blur=blur, noise=noise, jpeg=jpeg, tone=tone)
    for field, rows in given.items():
        if rows is not None:
            keep.append(_upload(field, rows, B, dev))
            setattr(d, field, keep[-1].data_ptr())
    return d, out, keep


def _preprocess(source, is_list, B, Hin, Win, out_size, flips, mean, std, jitter, affine, mosaic, window, letterbox, blur, persp, jpeg, tone,
                noise, dev):
    """The one call site of the chain: `preprocess_images` (packed) and `preprocess_image_list` (is_list) after their argument checks."""
    d, out, keep = _chain_desc(source, is_list, B, Hin, Win, out_size, flips, mean, std, jitter, affine, mosaic, window, letterbox, blur, persp,
                               jpeg, tone, noise, dev)
    lib = L.lib()
    ws = L.workspace(lib.sd_preprocess_chain_workspace_bytes(C.byref(d)), dev)   # (0 for a descriptor the call below refuses)
    L.check(lib.sd_preprocess_chain(C.byref(d), ws.data_ptr(), ws.numel(), L.stream()), "sd_preprocess_chain")
    del keep
    return out


def preprocess_images(images: torch.Tensor, out_size, flips=None, mean=_MEAN, std=_STD, jitter=None, affine=None, mosaic=None,
                      window=None, letterbox=None, blur=None, persp=None, jpeg=None, tone=None, noise=None) -> torch.Tensor:
    """images: (B, Hin, Win, 3) uint8 on the GPU; out_size = (width, height); flips: (B,) uint8 (bit 0 horizontal, bit 1 vertical)
    or None; jitter: None or (order words (B,) int32, factors (B, 3) fp32) as `jitter_words` makes them; affine: None or B rows of the 6
    coefficients of `affine_inverse_matrix` at out_size (the warp runs on the resized image, in front of the jitter, fill `_FILL`); mosaic:
    None or (geom: B rows [cx, cy, s0 .. s3], matrices: B x 4 x 6) as `mosaic_tiles` makes them, the sources s_q indexing THIS batch
    (the composite is built from the resized images, in front of the warp); window: None or ((canvas width, canvas height), B origins
    (x0, y0)): the resize targets the canvas and only its out_size window at the origin is produced (`sd_preprocess_images_window`;
    origins are clamped into the canvas on the device), every later stage works on that window; letterbox: None or (wi, hi, px, py) as
    `letterbox_geometry` gives them: the resize targets wi x hi and the result is pasted at (px, py) into an out_size frame of `_FILL`
    (`sd_preprocess_images_letterbox`), every later stage works on that frame (not together with `window`); blur: None or B rows
    (R, ww, fw) as `blur_box_params` makes them: Pillow's GaussianBlur after the warp, in front of the jitter
    (`sd_preprocess_images_blur`, chosen only when blur is set; a row of r = 0 leaves its image as it is); persp: None or B rows of the 8
    coefficients of `perspective_coeffs` / `compose_affine_perspective` at out_size: the warp is that homography (`sd_preprocess_images_persp`,
    chosen only when persp is set; not together with `affine`, which the caller folds in); jpeg: None or B rows [on, ql[64], qc[64]] as
    `jpeg_rows` makes them: Pillow's JPEG round trip after the blur, in front of the jitter (`sd_preprocess_images_jpeg`, chosen only when
    jpeg is set; height and width multiples of 16; a row of quality 0 leaves its image as it is); tone: None or B rows [mode, cut_lo, cut_hi,
    0] as `tone_rows` makes them: Pillow's autocontrast or equalize after the JPEG round trip, in front of the jitter
    (`sd_preprocess_images_tone`, chosen only when tone is set; any size; a row of mode 0 leaves its image as it is); noise: None or B rows
    [k0, k1, a, b] as `noise_rows` makes them: the sensor noise after the blur, in front of the JPEG round trip
    (`sd_preprocess_images_noise`, chosen only when noise is set; any size; a row with a = b = 0 leaves its image as it is).
    Returns (B, 3, height, width) fp32 = Normalize(to_tensor(flip(jitter(tone(jpeg(noise(blur(affine(mosaic(resize(image))))))))))) of
    transforms.py:217-226."""
    L.require_cuda(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise L.SdError(f"preprocess_images expects (B, H, W, 3) uint8, got {tuple(images.shape)} {images.dtype}")
    images = images.contiguous()
    B, Hin, Win, _ = images.shape
    return _preprocess(images.data_ptr(), False, B, Hin, Win, out_size, flips, mean, std, jitter, affine, mosaic, window, letterbox, blur, persp,
                       jpeg, tone, noise, images.device)


def preprocess_image_list(pointers: torch.Tensor, hin: int, win: int, out_size, flips=None, mean=_MEAN, std=_STD, jitter=None,
                          affine=None, mosaic=None, window=None, letterbox=None, blur=None, persp=None, jpeg=None, tone=None, noise=None) -> torch.Tensor:
    """`preprocess_images` over B images that are not packed together: pointers is a (B,) int64 DEVICE tensor of the device addresses of
    B (hin, win, 3) uint8 images (any byte alignment; the caller keeps them alive until the work on the current stream is done), e.g. entries
    of data/image_cache.py's DeviceImageCache.  Same arguments otherwise, same output bytes as `preprocess_images` on the stacked images."""
    L.require_cuda(pointers)
    if pointers.dtype != torch.int64 or pointers.dim() != 1 or pointers.numel() == 0:
        raise L.SdError(f"preprocess_image_list expects a non-empty (B,) int64 pointer table, got {tuple(pointers.shape)} {pointers.dtype}")
    pointers = pointers.contiguous()
    return _preprocess(pointers.data_ptr(), True, pointers.numel(), int(hin), int(win), out_size, flips, mean, std, jitter, affine, mosaic, window,
                       letterbox, blur, persp, jpeg, tone, noise, pointers.device)


def transpose_select(batch: torch.Tensor, select) -> torch.Tensor:
    """(B, P, S, S) fp32 on the GPU -> a new tensor: image b transposed (x and y swapped) where `select[b] & 1`, copied otherwise
    (`sd_transpose_select`, one launch).  select: B flags (a sequence, or a uint8 tensor on either side)."""
    L.require_cuda(batch)
    x = batch.contiguous().float()
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise L.SdError(f"transpose_select expects a (B, P, S, S) batch of square images, got {tuple(x.shape)}")
    B, P, S, _ = x.shape
    sel = torch.as_tensor(select, dtype=torch.uint8).to(x.device, non_blocking=True)
    if sel.numel() != B:
        raise L.SdError("select must have one entry per image")
    out = torch.empty_like(x)
    L.check(L.lib().sd_transpose_select(x.data_ptr(), out.data_ptr(), B, P, S, sel.data_ptr(), L.stream()), "sd_transpose_select")
    return out


def jitter_words(order, brightness, contrast, saturation, hue):
    """One image's ColorJitter parameters in the form `sd_preprocess_images_jitter` takes: the op order (a permutation of
    0 brightness, 1 contrast, 2 saturation, 3 hue) packed two bits each, the hue shift byte `uint8(hue * 255)` torchvision's adjust_hue
    adds to the H channel (truncation toward zero, wrap-around) in bits 8-15, and the three blend factors."""
    word = sum(int(op) << (2 * k) for k, op in enumerate(order)) | ((int(hue * 255) & 0xFF) << 8)
    return word, (float(brightness), float(contrast), float(saturation))


class _Objects:
    """The object list an annotation had at some point (mosaic_annotation reads `objects` only)."""

    def __init__(self, objects):
        self.objects = list(objects)


# The draw steps of one batch, in the order in which they consume torch's global generator: the only place that order is written
# (`draw_all` runs them, `Draws` names their answers).  A step that is off draws nothing and answers None.
DRAW_STEPS = ("draws_for", "affine_draws_for", "mosaic_draws_for", "window_draws_for", "transpose_draws_for", "blur_draws_for",
              "perspective_draws_for", "jpeg_draws_for", "tone_draws_for", "noise_draws_for")
Draws = namedtuple("Draws", ["base" if step == "draws_for" else step[:-len("_draws_for")] for step in DRAW_STEPS])     # base = (flips, jitter)
# One batch's draws and what is derived from them once: the affine matrices (source <- output and its forward twin), with a perspective draw
# the homographies they are folded into (then `inverse` is not passed on) and the perspective's forward twins, and the mosaic tiles.
_Plan = namedtuple("_Plan", "draws inverse forward6 homography forward8 tiles")


class ValidationAugmentation:
    """transforms.py:255-261 for a batch: Resize((width, height)) + Normalize (+ the clip Encode applies, transforms.py:154).  With
    `--keep_aspect` the Resize is a letterbox, its geometry computed per size group at the current size (`letterbox_geometry`)."""

    def __init__(self, args):
        self.args = args
        self.size = (args.width, args.height)
        self.keep_aspect = bool(getattr(args, "keep_aspect", False))

    def draws_for(self, n):
        """(flips, jitter) for n samples: validation draws nothing."""
        return None, None

    def _no_draw(self, n, groups=None):
        """Every other step of DRAW_STEPS (set below the class): validation has none of these stages and never draws."""
        return None

    def draw_all(self, n, groups):
        """The draws of a batch of n samples, every step of DRAW_STEPS in that order; groups = the index lists of its size groups."""
        return Draws(*(getattr(self, step)(n, groups) if step == "mosaic_draws_for" else getattr(self, step)(n) for step in DRAW_STEPS))

    @staticmethod
    def size_groups(images):
        """{(hin, win): (indices into the batch, stack of those images)} of what `__call__` accepts as `images`."""
        if hasattr(images, "groups"):                                # data/feeder.py GroupedBatch: grouped by size and uploaded already
            return images.groups
        if isinstance(images, torch.Tensor) and images.dim() == 4:
            return {tuple(images.shape[1:3]): (list(range(images.shape[0])), images)}
        by_size = {}
        for i, im in enumerate(images):
            t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
            by_size.setdefault(tuple(t.shape[:2]), []).append((i, t))
        return {k: ([i for i, _ in v], torch.stack([t for _, t in v])) for k, v in by_size.items()}

    def _resample(self, groups, size, tables, then=None):
        """One chain call per size group at `size` with the keyword tables `tables(idx, (win, hin))` gives, packed or by pointer list, and
        the results scattered to the samples' places: the (B, 3, height, width) tensor.  `then(idx, (win, hin))` runs behind each group's
        call: host work there is hidden behind the device's (the next group's first upload waits for this group's kernels)."""
        dev = self.args.device
        out = None
        for (hin, win), (idx, stack) in groups.items():
            if hasattr(stack, "pointers"):                           # data/image_cache.py ImageList: cached / uploaded images by address
                res = preprocess_image_list(stack.pointers, hin, win, size, **tables(idx, (win, hin)))
            else:
                res = preprocess_images(stack.to(dev, non_blocking=True), size, **tables(idx, (win, hin)))
            if len(groups) == 1:
                out = res
            else:
                if out is None:
                    out = torch.empty((sum(len(i) for i, _ in groups.values()), 3, size[1], size[0]), dtype=torch.float32, device=dev)
                out[torch.as_tensor(idx, device=dev)] = res
            if then is not None:
                then(idx, (win, hin))
        return out

    def images_at(self, images, size):
        """The Resize + Normalize of `__call__` at another `size` = (width, height), from the same SOURCE images: the
        (B, 3, height, width) tensor only.  No annotation is touched (`__call__` edits them in place, once) and nothing is drawn: this
        is the plain validation transform, what the multi-scale test (model/tta.py ScaleTta) runs at its extra sizes."""
        return self._resample(self.size_groups(images), tuple(size),
                              lambda idx, src: dict(letterbox=letterbox_geometry(src, tuple(size))) if self.keep_aspect else {})

    def _plan(self, n, groups):
        """The draws of one batch and what follows from them once per batch (_Plan), after the two refusals."""
        W, H = self.size
        d = self.draw_all(n, groups)
        inverse = forward6 = homography = forward8 = tiles = None
        if d.affine is not None:
            inverse = [affine_inverse_matrix((W, H), a, s, (tx, ty)) for a, s, tx, ty in d.affine]
            forward6 = [affine_forward_matrix((W, H), a, s, (tx, ty)) for a, s, tx, ty in d.affine]
        if d.perspective is not None:                                # the warp slot becomes one homography per image: affine, then perspective
            frame = [(0.0, 0.0), (float(W), 0.0), (float(W), float(H)), (0.0, float(H))]
            ident6, ident8 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
            homography = [compose_affine_perspective(ident6 if inverse is None else inverse[i], ident8 if quad is None else perspective_coeffs(frame, quad))
                          for i, quad in enumerate(d.perspective)]
            forward8 = [None if quad is None else perspective_coeffs(quad, frame) for quad in d.perspective]
        if d.mosaic is not None:
            tiles = [mosaic_tiles((W, H), i, draw) for i, draw in enumerate(d.mosaic)]
        if d.transpose is not None and W != H:
            raise L.SdError(f"aug_transpose: a transposed sample needs a square batch, not {W} x {H}")
        if d.window is not None and self.keep_aspect:
            raise L.SdError("keep_aspect does not combine with train_tiles: a window is cut from the stretched canvas")
        return _Plan(d, inverse, forward6, homography, forward8, tiles)

    def _group_tables(self, plan, idx, src):
        """The keyword tables of one size group's chain call: the rows of its samples `idx`, in the group's order."""
        W, H = self.size
        d = plan.draws
        pick = lambda rows: [rows[i] for i in idx]
        kw = {}
        if d.base[0] is not None:
            kw["flips"] = pick(d.base[0])
        if d.base[1] is not None:
            kw["jitter"] = (pick(d.base[1][0]), pick(d.base[1][1]))
        if plan.homography is not None:                              # (the affine draw is folded in: `affine=` is not passed)
            kw["persp"] = pick(plan.homography)
        elif plan.inverse is not None:
            kw["affine"] = pick(plan.inverse)
        if plan.tiles is not None:                                   # the kernel's sources index this group's stack: partners come from the group
            where = {i: k for k, i in enumerate(idx)}
            kw["mosaic"] = ([[*plan.tiles[i][0][:2], *(where[s] for s in plan.tiles[i][0][2:])] for i in idx], [plan.tiles[i][1] for i in idx])
        if d.window is not None:
            kw["window"] = (d.window[0], pick(d.window[1]))
        for stage, rows_of in (("blur", lambda radii: [blur_box_params(r) for r in radii]), ("jpeg", jpeg_rows),
                               ("tone", lambda draws: tone_rows(draws, W * H)), ("noise", noise_rows)):
            if getattr(d, stage) is not None:                        # photometric: the annotations do not move; the cuts count pixels of the input
                kw[stage] = rows_of(pick(getattr(d, stage)))
        if self.keep_aspect:                                         # one geometry per size group, at the current (multi-scale) size
            kw["letterbox"] = letterbox_geometry(src, (W, H))
        return kw

    def _move_annotations(self, plan, annotations, idx, src):
        """The annotations of one size group (source size `src`) through what its images went through, in the images' order: 1 resize or
        letterbox or window, 2 mosaic, 3 affine or affine + perspective, 4 hflip, 5 vflip, 6 transpose, 7 clip."""
        W, H = self.size
        d = plan.draws
        for i in idx:
            ann = annotations[i]
            ann.img_size = ann.img_size or src
            if self.keep_aspect:                                     # 1: to the inner image, then to its place in the frame: nothing leaves it
                letterbox_annotation(ann, src, (W, H))
            elif d.window is None:
                ann.resize(src, (W, H))                              # transforms.py:58
            else:                                                    # to the canvas, then into the window: what leaves it is dropped
                x0, y0 = d.window[1][i]
                ann.resize(src, d.window[0])
                affine_annotation(ann, [1.0, 0.0, -float(x0), 0.0, 1.0, -float(y0)], (W, H))
        if plan.tiles is not None:                                   # 2: an image is itself and maybe someone's partner: compose from the
            resized = {i: _Objects(annotations[i].objects) for i in idx}      # resized objects of the whole group, as they were
            for i in idx:
                if d.mosaic[i] is not None:
                    geom, _, forward, rects = plan.tiles[i]
                    mosaic_annotation(annotations[i], [resized[s] for s in geom[2:]], forward, rects)
        flips, transposes, affine, persp = d.base[0], d.transpose, plan.forward6, plan.forward8
        for i in idx:
            ann = annotations[i]
            forward6 = None if affine is None else affine[i]
            if persp is not None and persp[i] is not None:           # 3: affine, then perspective; one inside test at the end
                perspective_annotation(ann, persp[i], (W, H), affine_forward=forward6)
            elif forward6 is not None:                               # on the resized image, before the flips: drops what leaves the frame
                affine_annotation(ann, forward6, (W, H))
            if flips is not None and flips[i] & 1:
                hflip_annotation(ann, (W, H))                        # 4: transforms.py:15 (on the resized image)
            if flips is not None and flips[i] & 2:
                vflip_annotation(ann, (W, H))                        # 5: transforms.py:28
            if transposes is not None and transposes[i]:
                transpose_annotation(ann, (W, H))                    # 6: last, like the image's
            clip_annotation(ann, (W, H))                             # 7: transforms.py:154

    def __call__(self, images, annotations):
        """images: list of (H, W, 3) uint8 arrays / tensors (any sizes) or one (B, H, W, 3) tensor; annotations: list of
        ImageAnnotation in ORIGINAL image pixels (modified in place like the reference's Resize / flips / Encode clip do on their
        copies).  Returns ((B, 3, height, width) fp32 device tensor, annotations in network-input pixels)."""
        groups = self.size_groups(images)
        plan = self._plan(sum(len(idx) for idx, _ in groups.values()), [idx for idx, _ in groups.values()])
        out = self._resample(groups, tuple(self.size), lambda idx, src: self._group_tables(plan, idx, src),
                             then=lambda idx, src: self._move_annotations(plan, annotations, idx, src))
        if plan.draws.transpose is not None:                         # one launch over the assembled batch, after the flips
            out = transpose_select(out, plan.draws.transpose)
        return out, annotations


for _step in DRAW_STEPS[1:]:
    setattr(ValidationAugmentation, _step, ValidationAugmentation._no_draw)


class TrainAugmentation(ValidationAugmentation):
    """transforms.py:211-247: Resize + RandomColorJitter + RandomHorizontalFlip + RandomVerticalFlip + Normalize, and the per-epoch
    multi-scale `trigger_random_resize` (ratios 0.75 .. 1.25 in steps of 1/16, sizes rounded down to multiples of 32).  Random decisions
    have the reference's distributions -- ColorJitter.get_params (a random order of the four ops, brightness / contrast / saturation
    factors uniform in [1 - x, 1 + x], hue in [-x, x]), `randn < prob` for each flip (transforms.py:14,27: a normal, not a uniform,
    draw: the flip probability is Phi(0.5) = 0.69), `torch.randint` for the multi-scale ratio -- from torch's global generator (the
    reference draws them inside DataLoader worker processes with per-worker seeds: its stream is not reproducible across worker counts,
    so the distributions, not a draw order, are what there is to match).  The order in which one batch's steps consume the generator
    is DRAW_STEPS; every attribute a step reads (rotate .. noise_shot) is its `--aug_*` flag of utils/args.py AUG_FLAGS."""

    ratios = (0.75, 0.8125, 0.875, 0.9375, 1, 1.0625, 1.125, 1.1875, 1.25)
    brightness, contrast, saturation, hue = 0.25, 0.25, 0.15, 0.05            # transforms.py:38

    def __init__(self, args, prob=0.5):
        super().__init__(args)
        self.prob = prob
        for name, row in AUG_FLAGS.items():                          # rotate, scale, translate, mosaic, transpose, blur, perspective, jpeg, equalize,
            setattr(self, name[4:], type(row.default)(aug_flag(args, name)))    # autocontrast(_cutoff), noise(_shot): what the `*_draws_for` below read
        self.train_tiles = parse_tiles(getattr(args, "train_tiles", ""), "train_tiles")   # (Tx, Ty) of the canvas the windows are cut from, () = off
        self.tile_overlap = int(getattr(args, "tile_overlap", 64))

    def draws_for(self, n):
        """(flips, jitter) of n samples from torch's global generator, in THREE vectorised draws per batch: per-sample tiny tensor ops
        (the literal form of ColorJitter.get_params + the two flip draws: seven ops per sample) cost 450 ms per batch of 64 next to
        16 busy decode threads (measured: tools/feed_probe.py), 7 ms alone.  Same distributions: a uniformly random permutation of
        the four ops (argsort of four uniforms = torch.randperm(4)), brightness / contrast / saturation uniform in [1 - x, 1 + x], hue
        uniform in [-x, x] (uniform_(a, b) = a + (b - a) * U), each flip when a standard normal draw is below `prob`."""
        if self.args.no_augmentation:
            return None, None
        u = torch.rand(n, 8, dtype=torch.float64)
        z = torch.randn(n, 2)
        orders = torch.argsort(u[:, :4], dim=1).tolist()
        lo = torch.tensor([max(0.0, 1 - self.brightness), max(0.0, 1 - self.contrast), max(0.0, 1 - self.saturation), -self.hue], dtype=torch.float64)
        hi = torch.tensor([1 + self.brightness, 1 + self.contrast, 1 + self.saturation, self.hue], dtype=torch.float64)
        vals = (lo + (hi - lo) * u[:, 4:]).tolist()
        flip_bits = ((z[:, 0] < self.prob).to(torch.int64) | ((z[:, 1] < self.prob).to(torch.int64) << 1)).tolist()
        words, factors = [], []
        for order, (b, c, s_, h) in zip(orders, vals):
            w, f3 = jitter_words(order, b, c, s_, h)
            words.append(w); factors.append(f3)
        return flip_bits, (words, factors)

    def affine_draws_for(self, n):
        """(angle, scale, tx, ty) of n samples (torchvision RandomAffine.get_params' distributions, the shift left unrounded) from ONE draw
        on torch's global generator; None, and no draw at all, when the three ranges are 0 or
        augmentation is off.  The shift range follows the current multi-scale size."""
        if self.args.no_augmentation or (self.rotate == 0 and self.scale == 0 and self.translate == 0):
            return None
        W, H = self.size
        u = torch.rand(n, 4, dtype=torch.float64)
        lo = torch.tensor([-self.rotate, 1 - self.scale, -self.translate * W, -self.translate * H], dtype=torch.float64)
        hi = torch.tensor([self.rotate, 1 + self.scale, self.translate * W, self.translate * H], dtype=torch.float64)
        return [tuple(r) for r in (lo + (hi - lo) * u).tolist()]

    def mosaic_draws_for(self, n, groups):
        """Per sample None (not selected) or (cx, cy, (p1, p2, p3)) from ONE draw on torch's global generator, `rand(n, 6)` in float64:
        columns select (u < P), cx uniform over the integers of [W/4, 3W/4], cy over [H/4, 3H/4],
        and three partners.  groups = the index lists of the batch's size groups: partner k of image i is `idx[int(u * len(idx))]` of its
        own group idx (with replacement, i itself allowed: the device composes from the resized images of one group).  None, and no draw
        at all, with `--aug_mosaic 0` or augmentation off.  The centre follows the current multi-scale size."""
        if self.args.no_augmentation or self.mosaic == 0:
            return None
        W, H = self.size
        u = torch.rand(n, 6, dtype=torch.float64).tolist()
        draws = [None] * n
        for idx in groups:
            for i in idx:
                sel, ux, uy, *up = u[i]
                if sel < self.mosaic:
                    draws[i] = (W // 4 + int(ux * (W // 2 + 1)), H // 4 + int(uy * (H // 2 + 1)), tuple(idx[int(v * len(idx))] for v in up))
        return draws

    def window_draws_for(self, n):
        """((Wc, Hc), n origins (x0, y0)) with `--train_tiles`: the canvas `tile_canvas` gives for the current multi-scale size and, from ONE
        draw on torch's global generator, `rand(n, 2)` in float64, x0 = int(u (Wc - W + 1)) and
        y0 = int(u (Hc - H + 1)): uniform over the windows of the canvas.  None, and no draw at all, with the flag off.  The flag selects
        the pixel scale the network is trained at, not a perturbation of a sample, and a fixed window would hide most of every frame for
        good: the windows are drawn under `--no_augmentation` too."""
        if not self.train_tiles:
            return None
        W, H = self.size
        Wc, Hc = tile_canvas(W, H, self.train_tiles, self.tile_overlap)
        u = torch.rand(n, 2, dtype=torch.float64).tolist()
        return (Wc, Hc), [(int(ux * (Wc - W + 1)), int(uy * (Hc - H + 1))) for ux, uy in u]

    def transpose_draws_for(self, n):
        """n flags (1 where u < P) from ONE draw on torch's global generator, `rand(n)` in float64; None, and no draw at all, with `--aug_transpose 0` or augmentation off."""
        if self.args.no_augmentation or self.transpose == 0:
            return None
        return (torch.rand(n, dtype=torch.float64) < self.transpose).to(torch.uint8).tolist()

    def blur_draws_for(self, n):
        """n gaussian radii from ONE draw on torch's global generator, `rand(n, 2)` in float64: sample i is blurred when u0 < `prob`, with r = R * u1 in pixels of the current network input size (the same
        blur at every multi-scale size), else its radius is 0.0 (a copy row of the table).  None, and no draw at all, with `--aug_blur 0`
        or augmentation off."""
        if self.args.no_augmentation or self.blur == 0:
            return None
        u = torch.rand(n, 2, dtype=torch.float64).tolist()
        return [self.blur * u1 if u0 < self.prob else 0.0 for u0, u1 in u]

    def perspective_draws_for(self, n):
        """Per sample None (not selected) or the four output corners (tl, tr, br, bl) from ONE draw on torch's global generator,
        `rand(n, 9)` in float64: sample i is warped when u0 < `prob`; its corners are inset as
        torchvision's RandomPerspective insets them, in the continuous frame [0, W] x [0, H] of the current multi-scale size and left
        unrounded: tl = (u1 D W/2, u2 D H/2), tr = (W - u3 D W/2, u4 D H/2), br = (W - u5 D W/2, H - u6 D H/2), bl = (u7 D W/2,
        H - u8 D H/2).  The source quad is the frame's corners.  None, and no draw at all, with `--aug_perspective 0` or augmentation
        off."""
        if self.args.no_augmentation or self.perspective == 0:
            return None
        W, H = self.size
        d = self.perspective
        quads = []
        for u0, u1, u2, u3, u4, u5, u6, u7, u8 in torch.rand(n, 9, dtype=torch.float64).tolist():
            quads.append([(u1 * d * W / 2, u2 * d * H / 2), (W - u3 * d * W / 2, u4 * d * H / 2), (W - u5 * d * W / 2, H - u6 * d * H / 2),
                          (u7 * d * W / 2, H - u8 * d * H / 2)] if u0 < self.prob else None)
        return quads

    def jpeg_draws_for(self, n):
        """n JPEG qualities from ONE draw on torch's global generator, `rand(n, 2)` in float64: sample i is compressed when u0 < `prob`, at the quality min(95, QMIN + int(u1 (96 - QMIN))), uniform over
        the integers of [QMIN, 95]; else its quality is 0 (a copy row of the table).  None, and no draw at all, with `--aug_jpeg 0` or
        augmentation off."""
        if self.args.no_augmentation or self.jpeg == 0:
            return None
        u = torch.rand(n, 2, dtype=torch.float64).tolist()
        return [min(JPEG_MAX_QUALITY, self.jpeg + int(u1 * (JPEG_MAX_QUALITY + 1 - self.jpeg))) if u0 < self.prob else 0 for u0, u1 in u]

    def tone_draws_for(self, n):
        """n tone draws (mode, cutoff percent) from ONE draw on torch's global generator, `rand(n, 3)` in float64: sample i is equalized when u0 < `--aug_equalize`; otherwise it is autocontrasted when u1 < `--aug_autocontrast`,
        at the cutoff u2 `--aug_autocontrast_cutoff` percent; otherwise it is left alone -- never both.  None, and no draw at all, with both
        probabilities 0 or augmentation off."""
        if self.args.no_augmentation or (self.equalize == 0 and self.autocontrast == 0):
            return None
        u = torch.rand(n, 3, dtype=torch.float64).tolist()
        return [(TONE_EQUALIZE, 0.0) if u0 < self.equalize else
                (TONE_AUTOCONTRAST, self.autocontrast_cutoff * u2) if u1 < self.autocontrast else (TONE_COPY, 0.0) for u0, u1, u2 in u]

    def noise_draws_for(self, n):
        """n noise draws (k0, k1, sigma_read, gain) from TWO draws on torch's global generator:
        `rand(n, 3)` in float64 -- sample i is noised when u0 < 0.5, the flips' threshold, with sigma_read = u1 `--aug_noise` grey levels and
        gain = u2 `--aug_noise_shot` levels^2 per level -- then `randint(0, 2^32, (n, 2))` in int64, the two Philox key words of every sample.
        A sample that is not selected keeps its key and gets the strengths 0, 0: the identity row.  None, and no draw at all, with both flags
        0 or augmentation off."""
        if self.args.no_augmentation or (self.noise == 0 and self.noise_shot == 0):
            return None
        u = torch.rand(n, 3, dtype=torch.float64).tolist()
        keys = torch.randint(0, 2 ** 32, (n, 2), dtype=torch.int64).tolist()
        return [(k0, k1, u1 * self.noise, u2 * self.noise_shot) if u0 < self.prob else (k0, k1, 0.0, 0.0)
                for (u0, u1, u2), (k0, k1) in zip(u, keys)]

    def trigger_random_resize(self):
        if self.args.no_augmentation:
            return self.size
        ratio = self.ratios[torch.randint(len(self.ratios), (1,)).item()]
        self.size = (int(ratio * self.args.width / 32) * 32, int(ratio * self.args.height / 32) * 32)
        return self.size
