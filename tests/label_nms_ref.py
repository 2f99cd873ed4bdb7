"""The definition of the cross-label anchor suppression (`sd_label_nms`, and `LabelNms` around the bare network), restated three ways:

  * `expected_label_nms(P, R)`: torch ops, `torch.max` over the labels (its index is NOT used: the lowest label that attains the maximum is
    found by comparing), `max_pool2d(best, 2R+1, 1, R)` (which pads with -inf) and the lowest-label rule; any device;
  * `expected_nms5_labels(x, M, R)`: the project's own `clamped_sigmoid` / `nms` ops on the GPU, then `expected_label_nms` on the first M;
  * `loop_label_nms(P, R)`: a plain per-cell loop over numpy values, for the CPU test.

Only `max` and `==` enter the definition, so the kernel is compared with these bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F


def lowest_argmax(P):
    """(best (B,h,w), first (B,h,w) int64): the maximum over the labels and the LOWEST label that attains it."""
    best = P.max(dim=1).values
    M = P.shape[1]
    labels = torch.arange(M, device=P.device).view(1, M, 1, 1).expand_as(P)
    first = torch.where(P == best[:, None], labels, torch.full_like(labels, M)).min(dim=1).values
    return best, first


def expected_label_nms(P, R):
    """P (B,M,h,w) fp32 suppressed probability maps -> out[c] = P[c] where P[c] == win and c == first, else 0."""
    best, first = lowest_argmax(P)
    win = F.max_pool2d(best[:, None], 2 * R + 1, 1, R)                 # -inf padding: cells outside the map do not count
    M = P.shape[1]
    labels = torch.arange(M, device=P.device).view(1, M, 1, 1)
    keep = (P == win) & (labels == first[:, None])
    return torch.where(keep, P, torch.zeros_like(P))


def expected_nms5_labels(x, M, R):
    """Heatmap logits (B,C,h,w) on the GPU -> nms(clamped_sigmoid(x)) with `expected_label_nms` on the first M channels."""
    from structuredetector_amd.utils.ops import clamped_sigmoid, nms
    maps = nms(clamped_sigmoid(x))
    return torch.cat([expected_label_nms(maps[:, :M], R), maps[:, M:]], 1)


def loop_label_nms(P, R):
    """The definition cell by cell (numpy in, numpy out)."""
    P = np.asarray(P, np.float32)
    B, M, h, w = P.shape
    best = np.empty((B, h, w), np.float32)
    first = np.empty((B, h, w), np.int64)
    for b in range(B):
        for y in range(h):
            for x in range(w):
                m, a = P[b, 0, y, x], 0
                for c in range(1, M):
                    if P[b, c, y, x] > m:                              # strict: the lowest label keeps a tie
                        m, a = P[b, c, y, x], c
                best[b, y, x], first[b, y, x] = m, a
    out = np.zeros_like(P)
    for b in range(B):
        for y in range(h):
            for x in range(w):
                win = best[b, max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1].max()
                c = first[b, y, x]
                if P[b, c, y, x] == win:
                    out[b, c, y, x] = P[b, c, y, x]
    return out


def cpu_nms5(p):
    """(p == maxpool5x5(p)) * p with -inf padding on any device: the library's 5x5 rule, for inputs made on the CPU."""
    return torch.where(p == F.max_pool2d(p, 5, 1, 2), p, torch.zeros_like(p))


def tie_logits(shape, seed, device="cpu"):
    """The tie family: logits randint(-8, 9) * 0.5 (33 distinct values: equal peaks at different cells and under different labels)."""
    gen = torch.Generator("cpu").manual_seed(seed)
    return (torch.randint(-8, 9, shape, generator=gen).float() * 0.5).to(device)


def normal_logits(shape, seed, device="cpu"):
    gen = torch.Generator("cpu").manual_seed(seed)
    return (torch.randn(shape, generator=gen) * 2).to(device)
