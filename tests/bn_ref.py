"""fp64 references, launch-shape restatement and error bounds for the BatchNorm family and the column-sum machinery of
structuredetector_amd/csrc/sd_nn.hip (k_col_reduce<0|1|2>, k_rows_fold, col_pair_sums, the *_from_sums tails, k_bn_apply,
k_bn_bwd_apply, k_bn_fold and the bf16 x8 variants).  Plain numpy / torch-CPU: nothing here touches the GPU or the library.

Two input regimes (see docs/DESIGN_LOG.md, "BatchNorm and column sums: exact sums and fp64 bounds per branch"):

* exact: small integers and dyadic parameters, every fp32 partial sum and every elementwise result is exact -> tests assert equality;
* random: Gaussian activations with per-channel scale and offset -> tests assert the derived bounds below, per channel / per element.

Bounds (u = 2^-24, the unit roundoff of fp32):

* a per-channel sum of terms t_i: |got - ref| <= (L_red + L_fold + 2) * u * sum|t_i|.  A lane of k_col_reduce adds ceil(rpb / lanes) terms
  one after the other and thread rl == 0 adds the `lanes` lane sums: at most L_red - 2 roundings on any path; k_rows_fold the same with
  slab / lanes_f; everything after is fp64.  The remaining 4u cover the formation of a term in fp32 (x*x: one rounding; g * ((x - mean) *
  invstd): three) and the one rounding of an fp32 output.
* y = (x - mean) * invstd * gamma + beta + res:  6u * (|(x-mean)*invstd*gamma| + |beta| + |res|)  (five roundings, first order);
* dx = gamma * invstd * (g - mg - xhat * mgx):   8u * |gamma*invstd| * (|g| + |mg| + |xhat*mgx|)  (seven roundings);
* a bf16 store adds 2^-8 * |ref|; an fp64 expression rounded once to fp32 ("tail"): 2u * |ref|.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
BF16_U = 2.0 ** -8
EPS = 1e-5
MOMENTUM = float(np.float32(0.1))           # the ABI takes a float: the kernel sees 0.1f widened to double
SKIP_CAP = 1e-3                             # largest share of elements whose ReLU decision may be left unchecked

# (M, C) -> the branch of the host dispatch it is the smallest shape for
SHAPES = {
    "one_block_rows_lt_lanes": (7, 64),
    "c4_256_lanes_tail_block": (421, 4),
    "c1024_one_lane_f32_grid_stride": (4099, 1024),
    "rpb32_second_trip_no_fold": (40000, 8),
    "rpb64_ragged_f32_grid_stride": (70001, 64),
    "rpb128_bf16x8_grid_stride": (140003, 64),
    "rpb256_rows_fold_ragged_slab": (540001, 16),
}
# (rows, C) of synthetic partial rows for the finish kernels
ROW_CASES = {
    "one_row": (1, 4),
    "ragged_trip_65": (65, 64),
    "last_without_fold_2048": (2048, 4),
    "fold_one_lane_one_row_slab_2049": (2049, 512),
    "conv_epilogue_max_8192": (8192, 64),
    "wide_no_fold_six_trips_3000": (3000, 1024),
}


def cdiv(a, b):
    return -(-a // b)


# ---- the launch shape, restated from the host code (verified against the library on the GPU) ------------------------------------
def red_rows(M):
    r = 256
    while r > 16 and M // r < 1024:
        r >>= 1
    return r


def fold_rows(rows):
    return cdiv(rows, max(16, rows // 128)) if rows > 2048 else 0


def fold_plan(rows, C, scratch=True):
    """The k_rows_fold launch over `rows` partial rows of 2C floats, or None when the finish reads the rows directly."""
    if not scratch or fold_rows(rows) == 0 or 2 * C > 1024:
        return None
    slab = max(16, rows // 128)
    lanes = 256 // (2 * C // 4)
    return SimpleNamespace(slab=slab, rows_out=cdiv(rows, slab), lanes=lanes, L=cdiv(slab, lanes) + lanes)


def plan(M, C, elems=4):
    """Launch shape of a whole-tensor reduction over [M][C]; elems = 8 for k_col_reduce_bwd_bf16x8."""
    assert C % 4 == 0 and 4 <= C <= 1024 and 256 % (C // 4) == 0
    rpb = red_rows(M)
    nb = cdiv(M, rpb)
    lanes = 256 // (C // elems)
    fold = fold_plan(nb, C)
    L_red = cdiv(rpb, lanes) + lanes
    ws = ((nb + fold_rows(nb)) * 2 * C * 4 + 2 * C * 4 + 255) // 256 * 256
    return SimpleNamespace(rpb=rpb, nb=nb, lanes=lanes, L_red=L_red, fold=fold, L=L_red + (fold.L if fold else 0), workspace_bytes=ws,
                           trips=cdiv(fold.rows_out if fold else nb, 512))


def grid_stride_iterations(M, C, elems=4):
    """Iterations of the busiest thread of an apply kernel: ew_grid caps the grid at 4096 blocks of 256 threads."""
    return cdiv(M * C // elems, 4096 * 256)


def sum_bound(L, abs_sum):
    return (L + 2) * U * abs_sum


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def exact_params(C):
    c = torch.arange(C)
    third = torch.tensor([0.5, 1.0, 2.0])
    return SimpleNamespace(
        mean=((c % 5) - 2).float(), invstd=third[c % 3], gamma=third[(c // 3 + 1) % 3], beta=((c % 7) - 3).float() * 0.5,
        # dyadic "means" for an exact apply pass
        mg=((c % 3) - 1).float() * 0.5, mgx=((c % 4) - 2).float() * 0.25,
        # prior contents for accumulate = 1 and the running statistics
        prior0=((c % 9) - 4).float() * 0.5, prior1=((c % 11) - 5).float() * 0.5)


def exact_inputs(M, C, seed=0):
    """Small integers: every fp32 (and bf16) operand, product and partial sum is exact."""
    g = _gen(seed)
    d = exact_params(C)
    d.x = torch.randint(-3, 4, (M, C), generator=g).float()
    d.dy = torch.randint(-4, 5, (M, C), generator=g).float()
    d.res = torch.randint(-3, 4, (M, C), generator=g).float()
    d.y1 = torch.randint(-2, 3, (M, C), generator=g).float()                    # the relu = 1 input, zeros included
    d.maskbytes = torch.randint(0, 16, (M * C // 4,), generator=g).to(torch.uint8)
    return d


def random_params(C, seed=0, ratio=None):
    g = _gen(seed + 1000)
    c = torch.arange(C)
    sigma = 2.0 ** ((c % 8) - 4).double()
    r = torch.tensor([0.0, 1.0, 4.0], dtype=torch.float64)[c % 3] if ratio is None else torch.full((C,), float(ratio), dtype=torch.float64)
    mu = r * sigma * (1 - 2 * ((c // 3) % 2)).double()
    return SimpleNamespace(sigma=sigma, mu=mu, dyscale=2.0 ** ((c % 5) - 2).double(),
                           gamma=(torch.rand(C, generator=g) + 0.5), beta=torch.randn(C, generator=g),
                           prior0=torch.randn(C, generator=g), prior1=torch.rand(C, generator=g) + 0.5)


def random_inputs(M, C, seed=0, ratio=None, bf16=False):
    """x = sigma_c * N(0,1) + mu_c with sigma_c = 2^((c % 8) - 4) and |mu_c| / sigma_c cycled over {0, 1, 4} (or `ratio` everywhere);
    dy = N(0,1) * 2^((c % 5) - 2).  bf16: activations rounded to bf16 (the reference then starts from the rounded values).
    mean / invstd are the fp64 statistics of x rounded to fp32, as the forward hands them to the other passes."""
    g = _gen(seed)
    d = random_params(C, seed, ratio)
    rnd = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)
    d.x = rnd((torch.randn(M, C, generator=g).double() * d.sigma + d.mu).float())
    d.dy = rnd((torch.randn(M, C, generator=g).double() * d.dyscale).float())
    d.res = rnd(torch.randn(M, C, generator=g))
    S0, S1, _ = stats_sums(d.x)
    mean, invstd, _, _ = stats_tail(S0, S1, M, EPS)
    d.mean, d.invstd = mean.float(), invstd.float()
    return d


# ---- fp64 references ------------------------------------------------------------------------------------------------------------
def stats_sums(x):
    X = x.double()
    return X.sum(0), (X * X).sum(0), X.abs().sum(0)             # S0, S1 (= its own absolute sum), sum |x|


def stats_tail(S0, S1, n, eps, momentum=None, run_mean=None, run_var=None):
    """mean, invstd (biased variance) and the momentum update with the unbiased variance (biased when n == 1), as torch does."""
    S0, S1 = S0.double(), S1.double()
    mean = S0 / n
    var = (S1 / n - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    if run_mean is None:
        return mean, invstd, None, None
    unb = var * n / (n - 1.0) if n > 1 else var
    return mean, invstd, (1.0 - momentum) * run_mean.double() + momentum * mean, (1.0 - momentum) * run_var.double() + momentum * unb


def invstd_bound(S0, S1, b0, b1, n, eps):
    """|invstd(S0', S1') - invstd(S0, S1)| for |S0' - S0| <= b0, |S1' - S1| <= b1 (mean value theorem on (var + eps)^-1/2)."""
    mean = S0 / n
    var = (S1 / n - mean * mean).clamp_min(0.0) + float(np.float32(eps))
    bv = b1 / n + 2 * mean.abs() * b0 / n + (b0 / n) ** 2
    lo = (var - bv).clamp_min(1e-300)
    return torch.where(bv < var, 0.5 * bv * lo ** -1.5, torch.full_like(var, math.inf))


def pre_activation(x, mean, invstd, gamma, beta, res=None):
    """(pre, mag): pre = (x - mean) * invstd * gamma + beta [+ res], mag the sum of the absolute values of its three terms."""
    t = (x.double() - mean.double()) * invstd.double() * gamma.double()
    pre = t + beta.double()
    mag = t.abs_().add_(beta.double().abs())
    if res is not None:
        pre += res.double()
        mag += res.double().abs()
    return pre, mag


def pack_mask(bits):
    """[M][C] bool -> one byte per four consecutive elements, bit j = element j (what sd_bn_apply writes)."""
    b = bits.reshape(-1, 4).to(torch.uint8)
    return b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)


def unpack_mask(mask, M, C):
    m = mask.reshape(-1, 1)
    return torch.cat([(m >> j) & 1 for j in range(4)], 1).reshape(M, C).bool()


def bwd_terms(g, x, mean, invstd):
    """g and g * xhat in fp64 with their per-channel sums and absolute sums: (xhat, T0, T1, A0, A1)."""
    xhat = (x.double() - mean.double()) * invstd.double()
    t1 = g * xhat
    return xhat, g.sum(0), t1.sum(0), g.abs().sum(0), t1.abs().sum(0)


def bwd_apply(g, xhat, gamma, invstd, mg, mgx):
    """(dx, mag) = gamma * invstd * (g - mg - xhat * mgx) and |gamma * invstd| * (|g| + |mg| + |xhat * mgx|)."""
    k = gamma.double() * invstd.double()
    t = xhat * mgx.double()
    dx = k * (g - mg.double() - t)
    mag = k.abs() * (g.abs() + mg.double().abs() + t.abs_())
    return dx, mag


def bn_train_reference(x, gamma, beta, dy, res=None, relu=False, eps=EPS):
    """Training-mode BatchNorm [+ residual] [+ ReLU] forward and backward over [M][C], composed of the pieces above."""
    M = x.shape[0]
    S0, S1, _ = stats_sums(x)
    mean, invstd, _, _ = stats_tail(S0, S1, M, eps)
    pre, _ = pre_activation(x, mean, invstd, gamma, beta, res)
    y = pre.clamp_min(0.0) if relu else pre
    g = dy.double() * (pre > 0) if relu else dy.double()
    xhat, T0, T1, _, _ = bwd_terms(g, x, mean, invstd)
    dx, _ = bwd_apply(g, xhat, gamma, invstd, T0 / M, T1 / M)
    return SimpleNamespace(mean=mean, invstd=invstd, y=y, g=g, dx=dx, dgamma=T1, dbeta=T0)


def bn_fold(gamma, beta, rm, rv, eps=EPS):
    scale = gamma.double() / torch.sqrt(rv.double() + float(np.float32(eps)))
    return scale, beta.double() - rm.double() * scale


# ---- the summation order of the kernels in numpy fp32 (CPU check of the sum bound) ----------------------------------------------
def emulate_group_sums(t, group, lanes):
    """t [R][W] fp32 -> [ceil(R / group)][W] fp32: per group of `group` rows, lane l adds rows l, l + lanes, ... one after the other,
    then lane 0 adds the other lane sums in lane order (k_col_reduce and k_rows_fold)."""
    R, W = t.shape
    G, k = cdiv(R, group), cdiv(group, lanes)
    p = np.zeros((G, k * lanes, W), np.float32)
    flat = np.zeros((G * group, W), np.float32)
    flat[:R] = t
    p[:, :group] = flat.reshape(G, group, W)
    p = p.reshape(G, k, lanes, W)
    s = np.zeros((G, lanes, W), np.float32)
    for i in range(k):
        s = s + p[:, i]
    a = s[:, 0].copy()
    for l in range(1, lanes):
        a = a + s[:, l]
    return a


def emulate_column_sums(t, C, M=None):
    """fp64 per-channel sums of t [M][W] (W = C or 2C side by side) the way the library reduces [M][C]: blocks, fold, fp64."""
    p = plan(t.shape[0] if M is None else M, C)
    part = emulate_group_sums(np.ascontiguousarray(t, np.float32), p.rpb, p.lanes)
    if p.fold:
        part = emulate_group_sums(part, p.fold.slab, p.fold.lanes)
    return part.astype(np.float64).sum(0)
