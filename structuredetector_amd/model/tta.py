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
the logit domain."""
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


class FlipTta:
    """`net` behind flip test-time augmentation: `FlipTta(net, args, mode)(images)` returns the usual four-key output (a `TtaOutput`):
    `anchor_hm` / `part_hm` are the merged, suppressed PROBABILITY maps, `offsets` / `embeddings` view 0's (no copy).  Decode it with
    `tta_decoder(args)`."""

    def __init__(self, net, args, mode):
        if mode not in VIEW_FLIPS:
            raise L.SdError(f"unknown test-time augmentation mode {mode!r} (one of {', '.join(VIEW_FLIPS)})")
        self.net, self.args, self.mode = net, args, mode
        self.flips = VIEW_FLIPS[mode]
        self.label_count, self.part_count = len(args.labels), len(args.parts)

    def __call__(self, images):
        B = images.shape[0]
        M, nb = self.label_count, self.label_count + self.part_count
        out = self.net(tta_views(images, self.flips))
        if isinstance(out, torch.Tensor):                              # Network(raw_output=True)
            hm, offsets, embeddings = out[:, :nb], out[:, nb:nb + 2], out[:, nb + 2:nb + 4]
        else:
            a, p, offsets, embeddings = out["anchor_hm"], out["part_hm"], out["offsets"], out["embeddings"]
            if (a.dtype == p.dtype and a.stride() == p.stride() and a.shape[1] == M
                    and p.data_ptr() == a.data_ptr() + M * a.stride(1) * a.element_size()):
                hm = a.as_strided((a.shape[0], nb, a.shape[2], a.shape[3]), a.stride())      # adjacent slices of one head tensor: one launch
            else:
                hm = None
        if hm is not None:
            merged = tta_merge_nms(hm, self.flips)
            anchor_hm, part_hm = merged[:, :M], merged[:, M:]
        else:
            anchor_hm, part_hm = tta_merge_nms(a, self.flips), tta_merge_nms(p, self.flips)
        return TtaOutput(anchor_hm=anchor_hm, part_hm=part_hm, offsets=offsets[:B], embeddings=embeddings[:B])


def tta_decoder(args) -> FusedOutputDecoder:
    """The decoder that belongs with `FlipTta`: top-k directly on the merged, suppressed maps."""
    return FusedOutputDecoder(args)


def with_tta(net, decoder, args):
    """(net, decoder) as they are for `--tta none` (or no such attribute); otherwise `net` behind `FlipTta` and its decoder."""
    mode = getattr(args, "tta", "none") or "none"
    if mode == "none":
        return net, decoder
    return FlipTta(net, args, mode), tta_decoder(args)
