"""fp64 references, launch-shape restatement, inputs and error bounds for the pooling, stem-tail, upsample and cast kernels of
structuredetector_amd/csrc/sd_nn.hip (k_maxpool_fwd / _bwd / _fwd_bf16, k_bn_relu_maxpool_fwd[_pair], k_pool_bn_bwd_reduce[_quad],
k_pool_bn_bwd_apply[_quad], k_up2_bwd, k_cast_bf16 / _f32).  Plain numpy / torch-CPU: nothing here touches the GPU or the library.
Everything is NHWC; what tests/bn_ref.py already provides (U, BF16_U, SKIP_CAP, cdiv, fold_plan, sum_bound, exact_params, the random
inputs) is used from there.

The pool is MaxPool2d(3, stride 2, pad 1).  The winning tap of a window is its first maximum in row-major window order under strict `>`;
the tap number is r * 3 + s counted over the full 3x3 window, so the first in-bounds tap of a border window keeps its true number.  This
matches ATen for finite inputs only (an all -inf window keeps tap 0, NaN never wins): the tests use finite activations.

Two input regimes (docs/DESIGN_LOG.md, "Pooling, stem tail and upsample: exact taps and fp64 bounds per branch"):

* exact: small integers for x and dpool, the dyadic parameters of bn_ref.exact_params with gamma of both signs and one zero channel.  Every
  fp32 (and bf16) intermediate is exact with or without FMA contraction, ties are everywhere -> tests assert equality, taps included;
* random: Gaussian x with per-channel scale and offset, mean / invstd its batch statistics rounded to fp32, |gamma| in [0.5, 1.5] with
  alternating sign and one zero channel, beta ~ N(0, 1) -> tests assert the bounds below outside the ambiguous windows and elements.

Bounds (u = 2^-24):

* pooled value: the kernel evaluates pre = (x - mean) * invstd * gamma + beta in fp32 (four roundings, three with a fused last step), takes
  max(., 0) and maxima, all exact: |got - ref| <= 6u * (|(x - mean) * invstd * gamma| + |beta|) of the winning tap, as bn_ref's y bound;
* sums S0 = sum g, S1 = sum g * xhat: bn_ref.sum_bound(L, sum|term|) with L the fp32 additions on the longest path (bwd_plan): a term's
  g is gathered from up to four windows (GATHER_ADDS = 3 additions), a lane adds its terms one after the other (pixel form: ceil(256 /
  lanes) pixels; quad form: four per quad of ceil(64 / lanes) quads), thread rl == 0 adds the lane sums, k_rows_fold the same over a slab;
  the absolute sum takes |dpool| routed, so the gather's roundings are relative to it;
* dx = gamma * invstd * (g - mg - xhat * mgx) with A = sum|dpool routed| >= |g|: three roundings in g (3u A), one each in g - mg
  (u (A + |mg|)) and - t (u (A + |mg| + |t|)), three in t = xhat * mgx (3u |t|), two in the factor and the last product (2u of the whole):
  at most 7u A + 4u |mg| + 6u |t| <= 8u * |gamma * invstd| * (A + |mg| + |xhat * mgx|), the 8u bound of bn_ref.  The library's own
  mg / mgx differ from the reference's by the sum bound / n plus one rounding to fp32: |gamma * invstd| * (e_mg + |xhat| * e_mgx) more;
* a bf16 store adds BF16_U * |ref|;
* upsample backward: four additions of five terms, <= 4u * sum|terms| to first order: 5u * sum|terms|;
* plain pool backward: three additions: 4u * sum|dy routed|.

Ambiguity (random regime): with b = the pooled-value bound of an element, the kernel's post-ReLU value lies in [max(pre - b, 0),
max(pre + b, 0)].  An element's ReLU decision is ambiguous when |pre| <= b and gamma != 0 (gamma == 0: pre is beta exactly).  A window's
tap is ambiguous when some candidate and the winner have post-ReLU values that differ by a non-zero amount of at most the sum of their two
bounds, or are both zero in fp64 from different pre-activations while one of them is not certainly zero (pre + b > 0).  Exact fp64 ties
(the same x, or gamma == 0) are not ambiguous: the kernel sees the same tie.  Ambiguous windows / elements are left out of the tap, value
and dx comparisons, their |g| goes into the sum bounds, and their share must stay <= bn_ref.SKIP_CAP (tests/test_pool_ref_cpu.py).
"""
from types import SimpleNamespace

import numpy as np
import torch

from tests import bn_ref as R

U, BF16_U, SKIP_CAP, cdiv = R.U, R.BF16_U, R.SKIP_CAP, R.cdiv
RED_ROWS_PER_BLOCK = 256        # the pool reduction always takes 256 pixels (64 quads) per block, unlike red_rows(M) of the BatchNorm passes
GATHER_ADDS = 3                 # a pixel belongs to at most four windows
RANDOM_SEED = 1                 # of the random cases in tests/test_gpu_pool.py (the CPU test asserts their ambiguity share)

# (B, Hi, Wi, C) -> the branch it is the smallest shape for
FWD_SHAPES = {
    "single_one_window_one_tap": (1, 1, 1, 4),
    "pair_hi1_wi_odd_fifth_column_out": (1, 1, 3, 4),
    "single_wo3": (2, 5, 5, 8),
    "pair_wo4_wi_odd": (2, 5, 7, 8),
    "pair_two_blocks_ragged": (3, 6, 8, 64),
    "c12_bf16_single_f32_pair": (1, 4, 4, 12),
}
# expected kernel with the pair option on: (fp32, bf16)
FWD_KERNELS = {
    "single_one_window_one_tap": ("single", "single"),
    "pair_hi1_wi_odd_fifth_column_out": ("pair", "single"),        # C = 4: bf16 needs C % 8 == 0
    "single_wo3": ("single", "single"),
    "pair_wo4_wi_odd": ("pair", "pair"),
    "pair_two_blocks_ragged": ("pair", "pair"),
    "c12_bf16_single_f32_pair": ("pair", "single"),
}
BWD_SHAPES = {
    "quad_one_quad_256_lanes": (1, 2, 2, 4),
    "pixel_one_pixel": (1, 1, 1, 4),
    "pixel_odd_odd": (2, 5, 7, 8),
    "pixel_odd_even": (1, 3, 4, 64),
    "pixel_even_odd": (1, 4, 3, 64),
    "quad_two_blocks_ragged": (3, 10, 14, 64),
    "quad_c1024_one_lane": (1, 2, 2, 1024),
}
FOLD_SHAPES = {
    "quad_fold_2304_rows": (9, 256, 256, 4),
    "pixel_fold_2304_rows": (9, 255, 257, 4),
}
# output (B, H, W, C) of the upsample backward; the last one: 336 threads, a ragged second block
UP_SHAPES = {
    "one_thread": (1, 1, 1, 4),
    "odd_sizes": (2, 3, 5, 8),
    "c128": (2, 4, 6, 128),
    "two_blocks_ragged": (1, 3, 7, 64),
}
# the random cases of tests/test_gpu_pool.py: their ambiguity share is asserted on the CPU
RANDOM_CASES = sorted(set(FWD_SHAPES.values()) | set(BWD_SHAPES.values()))


def out_size(n):
    return (n + 2 - 3) // 2 + 1


# ---- the launch shape, restated from the host code ---------------------------------------------------------------------------------
def fwd_kernel(Wi, C, bf16, pair_option=True):
    """Which kernel sd_bn_relu_maxpool_fwd[_bf16] launches on 16-byte aligned buffers: two windows per thread or one."""
    pair = pair_option and out_size(Wi) % 2 == 0 and (not bf16 or C % 8 == 0)
    return "pair" if pair else "single"


def bwd_plan(B, Hi, Wi, C):
    """Launch shape of the fused backward's reduction and L, the fp32 additions on its longest path."""
    assert C % 4 == 0 and 4 <= C <= 1024 and 256 % (C // 4) == 0
    M = B * Hi * Wi
    nb = cdiv(M, RED_ROWS_PER_BLOCK)
    quad = Hi % 2 == 0 and Wi % 2 == 0
    lanes = 256 // (C // 4)
    per_lane = 4 * cdiv(RED_ROWS_PER_BLOCK // 4, lanes) if quad else cdiv(RED_ROWS_PER_BLOCK, lanes)
    L_red = per_lane + lanes
    fold = R.fold_plan(nb, C)
    return SimpleNamespace(M=M, nb=nb, quad=quad, lanes=lanes, per_lane=per_lane, L_red=L_red, fold=fold,
                           L=GATHER_ADDS + L_red + (fold.L if fold else 0))


# ---- fp64 references ----------------------------------------------------------------------------------------------------------------
def in_bounds(Hi, Wi):
    """[9][Ho][Wo] bool: tap r * 3 + s of window (oy, ox) lies inside the map."""
    Ho, Wo = out_size(Hi), out_size(Wi)
    oy, ox = torch.arange(Ho).view(Ho, 1), torch.arange(Wo).view(1, Wo)
    taps = []
    for r in range(3):
        for s in range(3):
            iy, ix = 2 * oy - 1 + r, 2 * ox - 1 + s
            taps.append((iy >= 0) & (iy < Hi) & (ix >= 0) & (ix < Wi))
    return torch.stack(taps)


def _candidates(x, pad):
    """[9][B][Ho][Wo][C]: the nine taps of every window, `pad` outside the map."""
    B, Hi, Wi, C = x.shape
    Ho, Wo = out_size(Hi), out_size(Wi)
    xp = torch.full((B, Hi + 2, Wi + 2, C), pad, dtype=x.dtype)
    xp[:, 1:Hi + 1, 1:Wi + 1] = x
    return torch.stack([xp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2] for r in range(3) for s in range(3)])


def first_max(cand):
    """Scan the taps in order, a later one wins only when strictly greater: (max, tap) with tap uint8."""
    m = torch.full(cand.shape[1:], -float("inf"), dtype=cand.dtype)
    idx = torch.zeros(cand.shape[1:], dtype=torch.uint8)
    for t in range(9):
        better = cand[t] > m
        m = torch.where(better, cand[t], m)
        idx = torch.where(better, torch.full_like(idx, t), idx)
    return m, idx


def tap_gather(plane, idx):
    """plane [B][Hi][Wi][C] at the pixel of every window's tap: [B][Ho][Wo][C] (idx must hold in-bounds taps)."""
    return _candidates(plane.double(), float("nan")).gather(0, idx.long().unsqueeze(0))[0]


def maxpool_fwd(x):
    return first_max(_candidates(x.double(), -float("inf")))


def maxpool_bwd(dy, idx, Hi, Wi):
    """Scatter every dy to the pixel of its window's tap."""
    B, Ho, Wo, C = dy.shape
    dxp = torch.zeros(B, Hi + 2, Wi + 2, C, dtype=torch.float64)
    for t in range(9):
        r, s = divmod(t, 3)
        dxp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2] += dy.double() * (idx == t)
    assert not dxp[:, 0].any() and not dxp[:, :, 0].any() and not dxp[:, Hi + 1:].any() and not dxp[:, :, Wi + 1:].any(), "out-of-bounds tap"
    return dxp[:, 1:Hi + 1, 1:Wi + 1].contiguous()


def pre_activation(x, mean, invstd, gamma, beta):
    """(pre, mag) = (x - mean) * invstd * gamma + beta and |(x - mean) * invstd * gamma| + |beta|."""
    t = (x.double() - mean.double()) * invstd.double() * gamma.double()
    return t + beta.double(), t.abs() + beta.double().abs()


def bn_relu_maxpool_fwd(x, mean, invstd, gamma, beta):
    pre, _ = pre_activation(x, mean, invstd, gamma, beta)
    y, idx = first_max(_candidates(pre.clamp_min(0.0), -float("inf")))
    return y, idx, pre


def maxpool_bn_relu_bwd(dpool, idx, x, mean, invstd, gamma, beta, mg=None, mgx=None):
    """The backward of max-pool -> ReLU -> BatchNorm(train) from a given tap plane.  mg / mgx default to S0 / n, S1 / n.  Also the absolute
    sums A0 = sum|dpool routed| (masked), A1 = sum|dpool routed| * |xhat| and routed_abs for the bounds."""
    B, Hi, Wi, C = x.shape
    n = B * Hi * Wi
    pre, _ = pre_activation(x, mean, invstd, gamma, beta)
    keep = pre > 0
    routed, routed_abs = maxpool_bwd(dpool, idx, Hi, Wi), maxpool_bwd(dpool.double().abs(), idx, Hi, Wi)
    g = routed * keep
    xhat = (x.double() - mean.double()) * invstd.double()
    S0, S1 = g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))
    ga = routed_abs * keep
    mg = S0 / n if mg is None else mg.double()
    mgx = S1 / n if mgx is None else mgx.double()
    k = gamma.double() * invstd.double()
    t = xhat * mgx
    dx = k * (g - mg - t)
    return SimpleNamespace(g=g, S0=S0, S1=S1, dgamma=S1, dbeta=S0, mg=mg, mgx=mgx, dx=dx, xhat=xhat, pre=pre, routed_abs=routed_abs,
                           A0=ga.sum((0, 1, 2)), A1=(ga * xhat.abs()).sum((0, 1, 2)), dx_mag=k.abs() * (ga + mg.abs() + t.abs()), k=k)


def upsample2x_bwd(dy, add=None):
    """dx[b, y, x] = sum of the 2x2 block of dy (+ add); also the sum of the absolute values of the terms."""
    B, H2, W2, C = dy.shape
    d = dy.double().view(B, H2 // 2, 2, W2 // 2, 2, C)
    dx, mag = d.sum((2, 4)), d.abs().sum((2, 4))
    if add is not None:
        dx, mag = dx + add.double(), mag + add.double().abs()
    return dx, mag


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _signs(C):
    """Alternating sign with channel 2 (and every 16th after it) exactly zero."""
    c = torch.arange(C)
    s = (1 - 2 * (c % 2)).float()
    s[2::16] = 0.0
    return s


def exact_inputs(B, Hi, Wi, C, seed=0):
    """Small integers and dyadic parameters: every fp32 / bf16 operand, product and partial sum is exact, ties are everywhere."""
    g = torch.Generator().manual_seed(seed)
    d = R.exact_params(C)
    d.gamma = d.gamma * _signs(C)
    Ho, Wo = out_size(Hi), out_size(Wi)
    d.x = torch.randint(-3, 4, (B, Hi, Wi, C), generator=g).float()
    d.dpool = torch.randint(-4, 5, (B, Ho, Wo, C), generator=g).float()
    return d


def random_inputs(B, Hi, Wi, C, seed=0, bf16=False):
    """x and the parameters as bn_ref.random_inputs over [B * Hi * Wi][C] (mean / invstd the batch statistics rounded to fp32), gamma with
    alternating sign and a zero channel; dpool = N(0, 1) * 2^((c % 5) - 2).  bf16: x and dpool rounded to bf16 first."""
    d = R.random_inputs(B * Hi * Wi, C, seed, bf16=bf16)
    d.x = d.x.view(B, Hi, Wi, C)
    d.gamma = (d.gamma * _signs(C)).float()
    d.beta = d.beta.float()
    g = torch.Generator().manual_seed(seed + 2000)
    Ho, Wo = out_size(Hi), out_size(Wi)
    dpool = (torch.randn(B, Ho, Wo, C, generator=g).double() * d.dyscale).float()
    d.dpool = dpool.bfloat16().float() if bf16 else dpool
    return d


def random_taps(B, Hi, Wi, C, seed=0):
    """A synthetic tap plane [B][Ho][Wo][C] uint8: every window draws uniformly among its in-bounds taps, so every route (window, tap) ->
    pixel occurs, the pixel four windows share and the border quads without a right or lower window included."""
    g = torch.Generator().manual_seed(seed + 3000)
    inb = in_bounds(Hi, Wi)                                     # [9][Ho][Wo]
    Ho, Wo = inb.shape[1:]
    count = inb.sum(0)                                          # >= 1: the centre tap is always inside
    k = (torch.rand(B, Ho, Wo, C, generator=g).double() * count.view(1, Ho, Wo, 1)).floor().long().clamp_max(8)
    k = torch.minimum(k, (count - 1).view(1, Ho, Wo, 1))
    order = inb.long().cumsum(0) - 1                            # rank of a tap among the in-bounds ones
    idx = torch.full((B, Ho, Wo, C), 255, dtype=torch.uint8)
    for t in range(9):
        hit = inb[t].view(1, Ho, Wo, 1) & (order[t].view(1, Ho, Wo, 1) == k)
        idx = torch.where(hit, torch.full_like(idx, t), idx)
    return idx


def window_class(Hi, Wi):
    """[Ho][Wo] int: bit 0 = the top row of the window is outside, bit 1 = bottom, bit 2 = left, bit 3 = right (0 = interior)."""
    inb = in_bounds(Hi, Wi)
    return (~inb[1]).long() | ((~inb[7]).long() << 1) | ((~inb[3]).long() << 2) | ((~inb[5]).long() << 3)


# ---- ambiguity (random regime) ------------------------------------------------------------------------------------------------------
def ambiguity(x, mean, invstd, gamma, beta):
    """(relu_unsure [B][Hi][Wi][C], tap_unsure [B][Ho][Wo][C], bound [B][Hi][Wi][C]) by the rule of the module docstring."""
    pre, mag = pre_activation(x, mean, invstd, gamma, beta)
    b = 6 * U * mag
    nz = (gamma != 0).view(1, 1, 1, -1)
    relu_unsure = (pre.abs() <= b) & nz
    inf = float("inf")
    cp, cb = _candidates(pre, -inf), _candidates(b, 0.0)       # outside the map: never a candidate
    ca = torch.where(cp > -inf, cp.clamp_min(0.0), cp)
    m, idx = first_max(ca)
    sel = idx.long().unsqueeze(0)
    wp, wb = cp.gather(0, sel)[0], cb.gather(0, sel)[0]         # the winner's pre-activation and bound
    tap_unsure = torch.zeros_like(idx, dtype=torch.bool)
    for t in range(9):
        inside = cp[t] > -inf
        diff = (m - ca[t]).abs()
        close = (diff > 0) & (diff <= cb[t] + wb)
        both_zero = (diff == 0) & (m == 0) & (cp[t] != wp) & ((cp[t] + cb[t] > 0) | (wp + wb > 0))
        tap_unsure |= inside & (close | both_zero)
    return relu_unsure, tap_unsure, b


# ---- the kernels' arithmetic in fp32, with and without a fused last step (CPU check of the exact regime) --------------------------
def f32_pre_activation(x, mean, invstd, gamma, beta, fused):
    """(x - mean) * invstd * gamma + beta in numpy fp32; fused: the last multiply-add rounded once (computed in fp64, exact for fp32
    operands up to one rounding)."""
    f = lambda t: t.numpy().astype(np.float32)
    p = (f(x) - f(mean)) * f(invstd)
    if fused:
        return torch.from_numpy((p.astype(np.float64) * f(gamma).astype(np.float64) + f(beta).astype(np.float64)).astype(np.float32))
    return torch.from_numpy(p * f(gamma) + f(beta))


def f32_dx(g, x, mean, invstd, gamma, mg, mgx, fused):
    """gamma * invstd * (g - mg - (x - mean) * invstd * mgx) in numpy fp32; fused: g - mg - t with t's product unrounded."""
    f = lambda t: t.numpy().astype(np.float32)
    xh = (f(x) - f(mean)) * f(invstd)
    if fused:
        inner = ((f(g) - f(mg)).astype(np.float64) - xh.astype(np.float64) * f(mgx).astype(np.float64)).astype(np.float32)
    else:
        inner = f(g) - f(mg) - xh * f(mgx)
    return torch.from_numpy(f(gamma) * f(invstd) * inner)
