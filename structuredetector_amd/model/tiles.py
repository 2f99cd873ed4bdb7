"""Tiled inference (`--tiles CxR`, `--tile_overlap PX`; no reference counterpart): a large image is shown to the network as overlapping
tiles of the network's own input size, the tile outputs are stitched into one large map, and that map is decoded once.

Every other inference path resizes the whole source image to one W x H network input; keypoints closer than a few output cells then merge
into one peak.  A larger `-W/-H` leaves the shapes the conv kernels are tuned for, grows the activations with the frame, and shows the
network a padding / context geometry it was never trained on.  Per batch of B images, with a grid of Tx x Ty tiles and an overlap of O
pixels (o = O / down_ratio cells):

  1. the canvas, (B, 3, Hc, Wc) with Wc = Tx*W - (Tx-1)*O and Hc = Ty*H - (Ty-1)*O, is resampled from the SOURCE images by the existing
     preprocess (`at_size((Wc, Hc))`), never from the base tensor;
  2. `sd_tile_views`: one launch writes the (T*B, 3, H, W) batch -- tile t = j*Tx + i of image b at index t*B + b (f6's ordering), tile
     (j, i) starting at pixel (j*(H-O), i*(W-O));
  3. the forward, through whatever `net` is set up for (fp32 or `--bf16_inference`), in chunks of at most max(B, 64) images so that the
     activation memory does not grow with T;
  4. `sd_tile_merge_nms`: one launch blends the clamped sigmoids of the covering tiles with a linear ramp across every seam, suppresses
     the blended canvas map (5x5 NMS) and copies offsets and embeddings from the owner tile (both are translation-invariant).

The result is a `TtaOutput` whose four maps are on the canvas grid; `TiledOutputDecoder` decodes it with the TILE's linkage radius and
reports network-input pixels (W x H).  Tiling shows objects at a larger pixel scale than whole-frame training did: train for it with
`train --train_tiles` (windows of the same canvas; data/augment.py).  No accuracy figure is claimed."""
from __future__ import annotations

import torch

from .. import _lib as L
from ..data.decoders import TiledOutputDecoder, TtaOutput
from ..utils.args import MAX_TILES, check_tile_overlap, tile_canvas
from .tta import _ViewNet

CHUNK = 64                          # images per forward of the tile batch, when the batch itself is not larger


def _grid(grid):
    tx, ty = (int(v) for v in grid)
    if not (1 <= tx <= MAX_TILES and 1 <= ty <= MAX_TILES):
        raise L.SdError(f"tiles: {tx} x {ty} (1 to {MAX_TILES} tiles per axis are supported)")
    return tx, ty


def tile_views(canvas: torch.Tensor, grid, overlap_px: int) -> torch.Tensor:
    """(B, 3, Hc, Wc) fp32 canvas -> (T*B, 3, H, W): tile t = j*Tx + i of image b at index t*B + b (`sd_tile_views`, one launch).
    grid = (Tx, Ty); the tile size follows from the canvas: W = (Wc + (Tx-1)*O) / Tx."""
    L.require_cuda(canvas)
    x = canvas.contiguous().float()
    if x.dim() != 4 or x.shape[1] != 3:
        raise L.SdError(f"tile_views expects a (B, 3, Hc, Wc) canvas, got {tuple(x.shape)}")
    tx, ty = _grid(grid)
    O = int(overlap_px)
    B, _, Hc, Wc = x.shape
    H, W = (Hc + (ty - 1) * O) // ty, (Wc + (tx - 1) * O) // tx
    out = torch.empty((tx * ty * B, 3, max(H, 1), max(W, 1)), dtype=torch.float32, device=x.device)
    L.check(L.lib().sd_tile_views(x.data_ptr(), out.data_ptr(), B, Hc, Wc, H, W, ty, tx, O, L.stream()), "sd_tile_views")
    return out


def tile_merge_nms(hm_view: torch.Tensor, reg_view, grid, overlap_cells: int):
    """Heatmap logits (T*B, C, h, w) and regression channels (T*B, R, h, w) or None of the tile forwards (channel-slice views pass
    without a copy) -> (out_hm (B, C, hc, wc), out_reg (B, R, hc, wc) or None): the blended, suppressed probability map on the canvas
    grid and the owner tiles' regressions, one launch (`sd_tile_merge_nms`)."""
    L.require_cuda(hm_view)
    tx, ty = _grid(grid)
    o = int(overlap_cells)
    T = tx * ty
    t, p, sb, sc = L.map_view(hm_view)
    TB, Cc, h, w = t.shape
    if TB % T:
        raise L.SdError(f"tile_merge_nms: {TB} images are not {T} tiles of a batch")
    B = TB // T
    hc, wc = ty * h - (ty - 1) * o, tx * w - (tx - 1) * o
    R, r, rp, r_sb, r_sc, out_reg = 0, None, None, 0, 0, None
    if reg_view is not None and reg_view.shape[1] > 0:
        L.require_cuda(reg_view)
        r, rp, r_sb, r_sc = L.map_view(reg_view)
        if (r.shape[0], r.shape[2], r.shape[3]) != (TB, h, w) or r.device != t.device:
            raise L.SdError(f"tile_merge_nms: heatmaps {tuple(t.shape)} and regressions {tuple(r.shape)} disagree")
        R = r.shape[1]
        out_reg = torch.empty((B, R, max(hc, 1), max(wc, 1)), dtype=torch.float32, device=t.device)
    out_hm = torch.empty((B, Cc, max(hc, 1), max(wc, 1)), dtype=torch.float32, device=t.device)
    L.check(L.lib().sd_tile_merge_nms(p, sb, sc, Cc, rp, r_sb, r_sc, R, out_hm.data_ptr(), out_reg.data_ptr() if R else None,
                                      B, h, w, ty, tx, o, L.stream()), "sd_tile_merge_nms")
    return out_hm, out_reg


def _regressions(offsets, embeddings):
    """Offsets + embeddings as ONE (no-copy) four-channel view when they are adjacent slices of one head tensor, else their concatenation."""
    o, e = offsets, embeddings
    if (o.dtype == e.dtype and o.stride() == e.stride() and o.shape[1] == 2 and e.shape[1] == 2
            and e.data_ptr() == o.data_ptr() + 2 * o.stride(1) * o.element_size()):
        return o.as_strided((o.shape[0], 4, o.shape[2], o.shape[3]), o.stride())
    return torch.cat([o, e], 1)


class TiledNet(_ViewNet):
    """`net` behind tiled inference: `TiledNet(net, args, grid, overlap)(images, at_size=f)` -- `images` the batch at the network input
    size (it only supplies B), `f((width, height))` the same source images resized + normalised to another size -- returns a `TtaOutput`
    whose four maps are on the canvas grid.  grid = (Tx, Ty), overlap in pixels.  `needs_sources` tells the callers to pass `at_size`.
    Decode it with `tiled_decoder(args, grid, overlap)`."""

    needs_sources = True

    def __init__(self, net, args, grid, overlap):
        self.grid = _grid(grid)
        W, H = int(args.width), int(args.height)
        try:
            self.overlap = check_tile_overlap(overlap, W, H)
        except ValueError as e:
            raise L.SdError(str(e)) from None
        self.overlap_cells = int(self.overlap // args.down_ratio)
        super().__init__(net, args)
        self.size = (W, H)
        self.canvas = tile_canvas(W, H, self.grid, self.overlap)

    def __call__(self, images, at_size=None):
        if at_size is None:
            raise L.SdError("TiledNet resamples its canvas from the source images: call it with at_size=(a callable (width, height) -> the "
                            "preprocessed batch at that size); a preprocessed tensor alone is not enough")
        B = images.shape[0]
        Wc, Hc = self.canvas
        canvas = at_size((Wc, Hc))
        if tuple(canvas.shape) != (B, 3, Hc, Wc):
            raise L.SdError(f"TiledNet: at_size({(Wc, Hc)}) returned {tuple(canvas.shape)}, expected {(B, 3, Hc, Wc)}")
        tiles = tile_views(canvas, self.grid, self.overlap)
        chunk = max(B, CHUNK)
        parts = [self.head_parts(tiles[i:i + chunk]) for i in range(0, tiles.shape[0], chunk)]
        if len(parts) == 1:
            heat, offsets, embeddings = parts[0]
            reg = _regressions(offsets, embeddings)
        else:                                                          # head tensors are small: the chunks are concatenated
            heat = [torch.cat([torch.cat(p[0], 1) for p in parts])]
            reg = torch.cat([torch.cat([p[1], p[2]], 1) for p in parts])
        reg_out = []

        def merge(hms):                                                # the regressions ride with the first launch
            hm, r = tile_merge_nms(hms[0], None if reg_out else reg, self.grid, self.overlap_cells)
            reg_out.append(r)
            return hm

        anchor_hm, part_hm = self.merged([heat], merge)
        return TtaOutput(anchor_hm=anchor_hm, part_hm=part_hm, offsets=reg_out[0][:, :2], embeddings=reg_out[0][:, 2:4])


def tiled_decoder(args, grid, overlap) -> TiledOutputDecoder:
    """The decoder that belongs with `TiledNet(net, args, grid, overlap)` (overlap in pixels)."""
    return TiledOutputDecoder(args, _grid(grid), int(int(overlap) // args.down_ratio))
