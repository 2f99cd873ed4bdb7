"""The definitions of the transposed-view entry points (`sd_d4_views`, `sd_d4_merge_nms`, `sd_transpose_select`), restated with torch ops
and the project's own `clamped_sigmoid` / `nms` (after `expected_merge` in tests/test_gpu_tta.py).  Works on either device."""
import torch


def flip(t, f):
    """bit 0 = horizontal (last axis), bit 1 = vertical."""
    dims = ([3] if f & 1 else []) + ([2] if f & 2 else [])
    return torch.flip(t, dims) if dims else t


def expected_views(x, flips):
    """(plain views, transposed views): view v of image b at index v*B + b; the transposed image is flipped, not the flipped one transposed."""
    xt = x.transpose(-1, -2)
    return torch.cat([flip(x, f) for f in flips]), torch.cat([flip(xt, f) for f in flips]).contiguous()


def expected_sum(x, xt, flips, sigmoid):
    """(sum_v flip_v(sigmoid(x_v)) + sum_v flip_v(sigmoid(xt_v)).transpose(-1, -2)) * (1 / (2 Vf)): each sum from its view 0 in view order,
    then the two sums added, fp32, every operation rounded on its own."""
    Vf = len(flips)
    B = x.shape[0] // Vf
    s, st = sigmoid(x.clone()), sigmoid(xt.clone())                # (whole tensors, freshly allocated: the library's sigmoid wants 16-byte aligned planes)
    a = t = None
    for v, f in enumerate(flips):
        sv, tv = flip(s[v * B:(v + 1) * B], f), flip(st[v * B:(v + 1) * B], f)
        a = sv if a is None else a + sv
        t = tv if t is None else t + tv
    return (a + t.transpose(-1, -2)) * (1.0 / (2 * Vf))


def expected_merge(x, xt, flips):
    from structuredetector_amd.utils import clamped_sigmoid, nms
    return nms(expected_sum(x, xt, flips, clamped_sigmoid).contiguous())


def expected_transpose_select(x, sel):
    return torch.stack([x[b].transpose(-1, -2) if sel[b] & 1 else x[b] for b in range(x.shape[0])]).contiguous()
