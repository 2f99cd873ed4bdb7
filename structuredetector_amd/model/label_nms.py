"""Cross-label anchor suppression (`--label_nms R`; no reference counterpart): the decoder suppresses peaks per heatmap channel only, so
an ambiguous object that peaks in two label maps at the same place, or a cell apart, becomes two objects.  With the flag, after the
per-label 5x5 NMS a peak of the anchor maps survives only where it equals the maximum over ALL labels within R cells:

    best(y, x) = max_c P[c, y, x];   first(y, x) = the lowest c that attains it;   win(y, x) = max of best over |dy|, |dx| <= R
    out[c, y, x] = P[c, y, x] if P[c, y, x] == win(y, x) and c == first(y, x) else 0

on the suppressed probability maps P (`sd_label_nms`).  Only `max` and `==`: equal values at different cells of a window both survive, as
in the 5x5 rule; a tie of labels at one cell goes to the lowest label; the rule is one max-pool, not a greedy loop (a peak suppressed by
a neighbour still suppresses).  With one label and R <= 2 nothing changes; with R > 2 peaks of one label closer than R are thinned too,
which is the wider window the tile scale needs.  Part maps are never touched: different part kinds legitimately share a location.

`LabelNms` wraps the network or any of the test-time wrappers (`FlipTta`, `ScaleTta`, `TransposeTta`, `TiledNet`), `with_tta` applies it
last.  Not consulted by `train` (the validation pass included) nor by the export."""
from __future__ import annotations

import torch

from .. import _lib as L
from ..data.decoders import TtaOutput
from .tta import _ViewNet, head_parts

MAX_RADIUS = 8                      # sd_label_nms takes R = 1 .. 8


def label_nms(maps: torch.Tensor, R: int) -> torch.Tensor:
    """Suppressed anchor probability maps (B, M, h, w) (a channel-slice view passes without a copy) -> (B, M, h, w): the definition above,
    one launch (`sd_label_nms`)."""
    L.require_cuda(maps)
    t, p, sb, sc = L.map_view(maps)
    B, M, h, w = t.shape
    out = torch.empty((B, M, h, w), dtype=torch.float32, device=t.device)
    L.check(L.lib().sd_label_nms(p, sb, sc, out.data_ptr(), B, M, h, w, int(R), L.stream()), "sd_label_nms")
    return out


def nms5_sigmoid(heat: torch.Tensor) -> torch.Tensor:
    """Heatmap logits (B, C, h, w) (a channel-slice view passes without a copy) -> `nms(clamped_sigmoid(x))`, the logits read once
    (`sd_nms5` with the sigmoid fused)."""
    L.require_cuda(heat)
    t, p, sb, sc = L.map_view(heat)
    B, Cc, h, w = t.shape
    out = torch.empty((B, Cc, h, w), dtype=torch.float32, device=t.device)
    L.check(L.lib().sd_nms5(p, sb, sc, out.data_ptr(), B, Cc, h, w, 1, L.stream()), "sd_nms5")
    return out


class LabelNms(_ViewNet):
    """`inner` (the network, or a wrapper that returns a `TtaOutput`) behind the cross-label suppression of radius `R` cells:
    `LabelNms(inner, args, R)(images[, at_size=f])` returns a `TtaOutput`.  Around a wrapper only `anchor_hm` is replaced (by
    `label_nms(anchor_hm, R)`), the other three tensors are the wrapper's own objects.  Around the bare network the heatmap logits go
    through `sd_nms5` with the sigmoid fused (one launch over the M + N channels when they are adjacent slices of one head tensor, else
    one on the anchors and one on the parts) and the anchor maps of that through `label_nms`; offsets / embeddings are the head's own
    views.  Decode it with the decoder of `inner`'s output (`tta_decoder(args)` for the bare network)."""

    def __init__(self, inner, args, R):
        super().__init__(inner, args)
        if int(R) != R or not 1 <= R <= MAX_RADIUS:
            raise L.SdError(f"LabelNms: a radius of 1 .. {MAX_RADIUS} cells, got {R!r}")
        self.R = int(R)
        self.needs_sources = bool(getattr(inner, "needs_sources", False))

    def __call__(self, images, at_size=None):
        from .predictor import call_net
        out = call_net(self.net, images, at_size)
        if isinstance(out, TtaOutput):
            return TtaOutput(anchor_hm=label_nms(out["anchor_hm"], self.R), part_hm=out["part_hm"], offsets=out["offsets"],
                             embeddings=out["embeddings"])
        M = self.label_count
        heat, offsets, embeddings = head_parts(out, M, M + self.part_count)
        anchor_hm, part_hm = self.merged([heat], lambda hms: nms5_sigmoid(hms[0]))
        return TtaOutput(anchor_hm=label_nms(anchor_hm, self.R), part_hm=part_hm, offsets=offsets, embeddings=embeddings)
