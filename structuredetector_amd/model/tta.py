"""Flip test-time augmentation (`--tta`; no reference counterpart): the network runs on the image and on its mirror images, the
heatmaps of the views are averaged as probabilities, and the result is decoded once.

Training draws horizontal and vertical flips independently (`TrainAugmentation`), so a trained model has seen all four mirrorings of
its data.  Per batch of B images:

  1. `sd_tta_views`: one launch writes the (V*B, 3, H, W) batch -- view v of image b at index v*B + b, view 0 the image itself.  The
     flip acts on the preprocessed tensor (what `sd_preprocess_images(flips=)` produces): no second resample.
  2. ONE forward over the V*B batch, through whatever `net` is set up for (fp32 or `--bf16_inference`).
  3. `sd_tta_merge_nms`: one launch over the M + N heatmap channels of the raw head tensor: clamped sigmoid of every view at the
     mirrored coordinate, mean in view order, 5x5 NMS -> (B, M + N, h, w) suppressed probability maps.
  4. offsets and embeddings are VIEW 0's (channel-slice views of the head tensor, no copy): they are trained only at keypoint cells,
     and a keypoint whose sub-cell offset is 0 lands one cell over in a mirrored view, so the mirrored passes' regressions at the merged
     peak are not trustworthy (CenterNet's flip test makes the same choice).

The merged maps are probabilities, already suppressed: they are decoded by `FusedOutputDecoder` (`tta_decoder`), never pushed back into
the logit domain.

Multi-scale test (`--tta_scales`, `ScaleTta`): training draws its input size per epoch from the ratios 0.75 .. 1.25 rounded down to
multiples of 32 (`TrainAugmentation.trigger_random_resize`), so a trained model has seen those sizes too.  Per batch the SOURCE images are
resized + normalised to every size (each from the original pixels, like training; never from an already resized tensor), each size goes
through steps 1 and 2, and ONE launch (`sd_tta_scale_merge_nms`) resamples the S x V heatmaps to the base grid (bilinear, half-pixel
centres), averages them as probabilities and suppresses.  Offsets and embeddings are the base size's view 0: an embedding is in cells of
its own scale.

Transposed views (`--tta_transpose`, `TransposeTta`): the flips are four of the eight symmetries of the grid; the other four are the
transposes (quarter turns and diagonal mirrors), lossless like the flips.  `sd_d4_views` writes, for every flip view, the view and the same
flip of the TRANSPOSED image; a square input is one forward over 2*Vf*B images, any other two forwards (H x W and W x H);
`sd_d4_merge_nms` flips and transposes the heatmaps back, averages the 2*Vf probability maps and suppresses, in one launch.  Offsets and
embeddings are view 0's, as above."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from ..data.decoders import FusedOutputDecoder, TtaOutput

# per mode, the flips of the views (bit 0 = horizontal, bit 1 = vertical: the encoding of the preprocess `flips`); view 0 is the image
VIEW_FLIPS = {"hflip": (0, 1), "vflip": (0, 2), "hvflip": (0, 1, 2, 3)}
MODES = ("none",) + tuple(VIEW_FLIPS)


def tta_views(images: torch.Tensor, flips) -> torch.Tensor:
    """(B, 3, H, W) fp32 -> (V*B, 3, H, W): view v of image b at index v*B + b (`sd_tta_views`, one launch)."""
    L.require_cuda(images)
    x = images.contiguous().float()
    if x.dim() != 4 or x.shape[1] != 3:
        raise L.SdError(f"tta_views expects a (B, 3, H, W) batch, got {tuple(x.shape)}")
    B, _, H, W = x.shape
    out = torch.empty((len(flips) * B, 3, H, W), dtype=torch.float32, device=x.device)
    L.check(L.lib().sd_tta_views(x.data_ptr(), out.data_ptr(), B, H, W, len(flips), (C.c_ubyte * len(flips))(*flips), L.stream()),
            "sd_tta_views")
    return out


def tta_merge_nms(logits: torch.Tensor, flips) -> torch.Tensor:
    """Heatmap logits (V*B, C, h, w) of the views (a channel-slice view passes without a copy) -> (B, C, h, w):
    nms(mean over the views of the clamped sigmoid at the mirrored coordinate), one launch (`sd_tta_merge_nms`)."""
    L.require_cuda(logits)
    V = len(flips)
    t, p, sb, sc = L.map_view(logits)
    VB, Cc, h, w = t.shape
    if VB % V:
        raise L.SdError(f"tta_merge_nms: {VB} images are not {V} views of a batch")
    out = torch.empty((VB // V, Cc, h, w), dtype=torch.float32, device=t.device)
    L.check(L.lib().sd_tta_merge_nms(p, sb, sc, out.data_ptr(), VB // V, Cc, h, w, V, (C.c_ubyte * V)(*flips), L.stream()),
            "sd_tta_merge_nms")
    return out


def d4_views(images: torch.Tensor, flips, joint=False):
    """(B, 3, H, W) fp32 -> (plain views (Vf*B, 3, H, W), transposed views (Vf*B, 3, W, H)), view v of image b at index v*B + b of both:
    `flip_f(x)` and `flip_f(x.transpose(-1, -2))` (`sd_d4_views`, one launch).  flips: `VIEW_FLIPS[mode]`, or (0,) for one view.
    joint=True (H == W only): ONE (2*Vf*B, 3, H, W) batch, the plain views first."""
    L.require_cuda(images)
    x = images.contiguous().float()
    if x.dim() != 4 or x.shape[1] != 3:
        raise L.SdError(f"d4_views expects a (B, 3, H, W) batch, got {tuple(x.shape)}")
    B, _, H, W = x.shape
    if joint and H != W:
        raise L.SdError(f"d4_views: one joint batch needs a square input, got {W} x {H}")
    Vf = len(flips)
    buf = torch.empty((2 * Vf * B, 3, H, W), dtype=torch.float32, device=x.device)
    out, out_t = buf[:Vf * B], buf[Vf * B:].view(Vf * B, 3, W, H)
    L.check(L.lib().sd_d4_views(x.data_ptr(), out.data_ptr(), out_t.data_ptr(), B, H, W, Vf, (C.c_ubyte * Vf)(*flips), L.stream()), "sd_d4_views")
    return buf if joint else (out, out_t)


def d4_merge_nms(logits: torch.Tensor, logits_t: torch.Tensor, flips) -> torch.Tensor:
    """Heatmap logits of the plain views (Vf*B, C, h, w) and of the transposed views (Vf*B, C, w, h) (channel-slice views pass without a
    copy) -> (B, C, h, w): nms((sum_v flip_v(sigmoid(plain_v)) + sum_v flip_v(sigmoid(transposed_v)).transpose(-1, -2)) / (2 Vf)), one
    launch (`sd_d4_merge_nms`)."""
    L.require_cuda(logits, logits_t)
    Vf = len(flips)
    t, p, sb, sc = L.map_view(logits)
    tt, pt, sbt, sct = L.map_view(logits_t)
    VB, Cc, h, w = t.shape
    if VB % Vf or tuple(tt.shape) != (VB, Cc, w, h) or tt.device != t.device:
        raise L.SdError(f"d4_merge_nms: {tuple(t.shape)} and {tuple(tt.shape)} are not {Vf} views of a batch and their transposes")
    out = torch.empty((VB // Vf, Cc, h, w), dtype=torch.float32, device=t.device)
    L.check(L.lib().sd_d4_merge_nms(p, sb, sc, pt, sbt, sct, out.data_ptr(), VB // Vf, Cc, h, w, Vf, (C.c_ubyte * Vf)(*flips), L.stream()),
            "sd_d4_merge_nms")
    return out


MAX_SCALES = 5                      # sd_tta_scale_merge_nms takes up to 5 sizes


def scale_sizes(args, ratios):
    """The (width, height) input sizes of the multi-scale test, the base size first: every ratio r gives (int(r*W/32)*32, int(r*H/32)*32)
    -- `TrainAugmentation.trigger_random_resize`'s rule -- in the order given; sizes equal to the base or to an earlier one are dropped."""
    W, H = int(args.width), int(args.height)
    sizes = [(W, H)]
    for r in ratios:
        size = (int(r * W / 32) * 32, int(r * H / 32) * 32)
        if min(size) < 32:
            raise L.SdError(f"tta_scales: ratio {r} of {W} x {H} rounds to {size[0]} x {size[1]} (every side must be at least 32)")
        if size not in sizes:
            sizes.append(size)
    if len(sizes) > MAX_SCALES:
        raise L.SdError(f"tta_scales: {len(sizes)} distinct input sizes ({', '.join(f'{w} x {h}' for w, h in sizes)}); at most {MAX_SCALES} "
                        "(the base size included) are supported")
    return sizes


def tta_scale_merge_nms(logits, flips, base_hw) -> torch.Tensor:
    """S heatmap-logit tensors (V*B, C, hs, ws), one per scale (channel-slice views pass without a copy) -> (B, C, h, w) on the base grid
    `base_hw` = (h, w): nms(mean over scales and views of the bilinearly resampled clamped sigmoid), one launch
    (`sd_tta_scale_merge_nms`).  flips: the views of every scale (`VIEW_FLIPS[mode]`, or (0,) for one view)."""
    L.require_cuda(*logits)
    S, V = len(logits), len(flips)
    h, w = base_hw
    views = [L.map_view(t) for t in logits]
    VB, Cc = views[0][0].shape[:2]
    if VB % V:
        raise L.SdError(f"tta_scale_merge_nms: {VB} images are not {V} views of a batch")
    for t, *_ in views:
        if t.shape[:2] != (VB, Cc) or t.device != views[0][0].device:
            raise L.SdError(f"tta_scale_merge_nms: scales disagree: {[tuple(v[0].shape) for v in views]}")
    out = torch.empty((VB // V, Cc, h, w), dtype=torch.float32, device=views[0][0].device)
    L.check(L.lib().sd_tta_scale_merge_nms((C.c_void_p * S)(*[v[1] for v in views]), (C.c_int64 * S)(*[v[2] for v in views]),
                                           (C.c_int64 * S)(*[v[3] for v in views]), (C.c_int * S)(*[v[0].shape[2] for v in views]),
                                           (C.c_int * S)(*[v[0].shape[3] for v in views]), out.data_ptr(), VB // V, Cc, h, w, S, V,
                                           (C.c_ubyte * V)(*flips), L.stream()), "sd_tta_scale_merge_nms")
    return out


def head_parts(out, M, nb):
    """A forward's output -> ([heatmap tensors to merge], offsets, embeddings): the M + N heatmap channels as ONE (no-copy) tensor when
    they are adjacent slices of one head tensor, else [anchor_hm, part_hm]."""
    if isinstance(out, torch.Tensor):                                  # Network(raw_output=True)
        return [out[:, :nb]], out[:, nb:nb + 2], out[:, nb + 2:nb + 4]
    a, p = out["anchor_hm"], out["part_hm"]
    if (a.dtype == p.dtype and a.stride() == p.stride() and a.shape[1] == M
            and p.data_ptr() == a.data_ptr() + M * a.stride(1) * a.element_size()):
        return [a.as_strided((a.shape[0], nb, a.shape[2], a.shape[3]), a.stride())], out["offsets"], out["embeddings"]
    return [a, p], out["offsets"], out["embeddings"]


class _ViewNet:
    """What the wrappers around `net` share (`FlipTta`, `ScaleTta`, `TransposeTta`, `TiledNet` in model/tiles.py): the mode check, the flips
    of the views, the label / part counts, and the step from the forwards' heatmaps to the two merged maps."""

    modes = MODES                   # the modes the wrapper takes

    def __init__(self, net, args, mode="none"):
        if mode not in self.modes:
            raise L.SdError(f"unknown test-time augmentation mode {mode!r} (one of {', '.join(self.modes)})")
        self.net, self.args, self.mode = net, args, mode
        self.flips = VIEW_FLIPS.get(mode, (0,))
        self.label_count, self.part_count = len(args.labels), len(args.parts)

    def head_parts(self, x):
        """`head_parts` of the forward over `x`."""
        return head_parts(self.net(x), self.label_count, self.label_count + self.part_count)

    def merged(self, heat, merge):
        """heat: per forward (or per half of one), the heatmap list of `head_parts`; merge([one tensor of each]) -> the merged map.
        Returns (anchor_hm, part_hm): ONE launch over the M + N channels when every entry is one tensor (adjacent slices of a head
        tensor), else two, anchors first, entries that are one tensor split into their channel-slice views."""
        M = self.label_count
        if all(len(hm) == 1 for hm in heat):
            out = merge([hm[0] for hm in heat])
            return out[:, :M], out[:, M:]
        heat = [hm if len(hm) == 2 else [hm[0][:, :M], hm[0][:, M:]] for hm in heat]
        return merge([hm[0] for hm in heat]), merge([hm[1] for hm in heat])


class ScaleTta(_ViewNet):
    """`net` behind the multi-scale test, combined with the flip views of `mode` ("none": one view):
    `ScaleTta(net, args, sizes, mode)(images, at_size=f)` -- `images` the batch at the base size `sizes[0]`, `f((width, height))` the same
    source images resized + normalised to another size -- returns a `TtaOutput` like `FlipTta`: S forwards of V*B images, one merge
    launch, the base size's view-0 offsets / embeddings (no copy).  `needs_sources` tells the callers to pass `at_size`."""

    needs_sources = True

    def __init__(self, net, args, sizes, mode="none"):
        super().__init__(net, args, mode)
        sizes = [tuple(int(v) for v in s) for s in sizes]
        if not 1 <= len(sizes) <= MAX_SCALES or len(set(sizes)) != len(sizes) or any(v < 32 or v % 32 for s in sizes for v in s):
            raise L.SdError(f"ScaleTta: 1 to {MAX_SCALES} distinct (width, height) sizes, multiples of 32, base first; got {sizes}")
        self.sizes = sizes

    def __call__(self, images, at_size=None):
        if at_size is None and len(self.sizes) > 1:
            raise L.SdError("ScaleTta resamples every size from the source images: call it with at_size=(a callable (width, height) -> "
                            "the preprocessed batch at that size); a preprocessed tensor alone is not enough")
        B = images.shape[0]
        W0, H0 = self.sizes[0]
        if tuple(images.shape[2:]) != (H0, W0):
            raise L.SdError(f"ScaleTta: the batch is {images.shape[3]} x {images.shape[2]}, the base size {W0} x {H0}")
        heat, offsets, embeddings = [], None, None
        for i, size in enumerate(self.sizes):
            x = images if i == 0 else at_size(size)
            if tuple(x.shape) != (B, 3, size[1], size[0]):
                raise L.SdError(f"ScaleTta: at_size({size}) returned {tuple(x.shape)}, expected {(B, 3, size[1], size[0])}")
            hm, off, emb = self.head_parts(tta_views(x, self.flips) if len(self.flips) > 1 else x)
            heat.append(hm)
            if i == 0:
                offsets, embeddings = off[:B], emb[:B]
        base_hw = tuple(heat[0][0].shape[2:])
        anchor_hm, part_hm = self.merged(heat, lambda hms: tta_scale_merge_nms(hms, self.flips, base_hw))
        return TtaOutput(anchor_hm=anchor_hm, part_hm=part_hm, offsets=offsets, embeddings=embeddings)


class FlipTta(_ViewNet):
    """`net` behind flip test-time augmentation: `FlipTta(net, args, mode)(images)` returns the usual four-key output (a `TtaOutput`):
    `anchor_hm` / `part_hm` are the merged, suppressed PROBABILITY maps, `offsets` / `embeddings` view 0's (no copy).  Decode it with
    `tta_decoder(args)`."""

    modes = tuple(VIEW_FLIPS)

    def __init__(self, net, args, mode):
        super().__init__(net, args, mode)

    def __call__(self, images):
        B = images.shape[0]
        heat, offsets, embeddings = self.head_parts(tta_views(images, self.flips))
        anchor_hm, part_hm = self.merged([heat], lambda hms: tta_merge_nms(hms[0], self.flips))
        return TtaOutput(anchor_hm=anchor_hm, part_hm=part_hm, offsets=offsets[:B], embeddings=embeddings[:B])


class TransposeTta(_ViewNet):
    """`net` behind the transposed-view test, combined with the flip views of `mode` ("none": the image and its transpose):
    `TransposeTta(net, args, mode)(images)` returns a `TtaOutput` like `FlipTta`: the merged, suppressed PROBABILITY maps of 2*Vf views and
    view 0's offsets / embeddings (no copy).  A square batch is one forward over 2*Vf*B images, any other two forwards of Vf*B images, at
    H x W and at W x H.  Decode it with `tta_decoder(args)`."""

    def __call__(self, images):
        B, n = images.shape[0], len(self.flips) * images.shape[0]
        if images.shape[2] == images.shape[3]:
            heat, offsets, embeddings = self.head_parts(d4_views(images, self.flips, joint=True))
            heat, heat_t = [hm[:n] for hm in heat], [hm[n:] for hm in heat]
        else:
            plain, transposed = d4_views(images, self.flips)
            heat, offsets, embeddings = self.head_parts(plain)
            heat_t, _, _ = self.head_parts(transposed)
        anchor_hm, part_hm = self.merged([heat, heat_t], lambda hms: d4_merge_nms(hms[0], hms[1], self.flips))
        return TtaOutput(anchor_hm=anchor_hm, part_hm=part_hm, offsets=offsets[:B], embeddings=embeddings[:B])


def tta_decoder(args) -> FusedOutputDecoder:
    """The decoder that belongs with `FlipTta`: top-k directly on the merged, suppressed maps."""
    return FusedOutputDecoder(args)


def with_tta(net, decoder, args):
    """(net, decoder) as they are for `--tta none`, no `--tta_scales` and no `--tiles` (or no such attributes); `net` behind `FlipTta` for
    a flip mode alone; `net` behind `ScaleTta` when `--tta_scales` adds at least one input size.  Both come with `tta_decoder(args)`.
    `--tiles` (model/tiles.py) puts `net` behind `TiledNet` with its `tiled_decoder`, and is refused together with the other two.
    `--tta_transpose`, alone or with a flip mode, puts `net` behind `TransposeTta`; with `--tta_scales` or `--tiles` it is refused.
    `--label_nms R` (model/label_nms.py) comes last, around whatever the rules above gave: a wrapper keeps its decoder, the bare `net`
    gets `tta_decoder(args)` (a `LabelNms` output holds suppressed probabilities).  R = 0, or no such attribute: nothing is added."""
    inner, inner_decoder = _with_views(net, decoder, args)
    R = int(getattr(args, "label_nms", 0) or 0)
    if R == 0:
        return inner, inner_decoder
    from .label_nms import LabelNms
    return LabelNms(inner, args, R), (tta_decoder(args) if inner is net else inner_decoder)


def _with_views(net, decoder, args):
    """`with_tta` without `--label_nms`."""
    from ..utils.args import parse_tiles, parse_tta_scales
    mode = getattr(args, "tta", "none") or "none"
    ratios = parse_tta_scales(getattr(args, "tta_scales", "") or "")
    grid = parse_tiles(getattr(args, "tiles", "") or "")
    if getattr(args, "tta_transpose", False):
        if ratios or grid:
            raise L.SdError("--tta_transpose does not combine with --tta_scales / --tiles: the transposed views are merged on one grid at one "
                            "input size; drop one of them")
        return TransposeTta(net, args, mode), tta_decoder(args)
    if grid:
        if mode != "none" or ratios:
            raise L.SdError("--tiles does not combine with --tta / --tta_scales: the tile outputs are stitched as they are; drop one of them")
        from .tiles import TiledNet, tiled_decoder
        overlap = getattr(args, "tile_overlap", 64)
        return TiledNet(net, args, grid, overlap), tiled_decoder(args, grid, overlap)
    if ratios:
        sizes = scale_sizes(args, ratios)
        if len(sizes) > 1:
            return ScaleTta(net, args, sizes, mode), tta_decoder(args)
        print(f"tta_scales: every ratio of {', '.join(f'{r:g}' for r in ratios)} rounds to the base size {sizes[0][0]} x {sizes[0][1]}: "
              "single-scale inference")
    if mode == "none":
        return net, decoder
    return FlipTta(net, args, mode), tta_decoder(args)
