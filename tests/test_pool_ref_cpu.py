"""CPU checks of tests/pool_ref.py: the fp64 references against torch-CPU autograd in double (values, gradients and the winning taps
against max_pool2d's return_indices), the preconditions of the exact regime, the ambiguity share of every random case the GPU file uses,
the synthetic tap planes, and that every shape reaches the branch its id names."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R
from tests import pool_ref as P

ALL_BWD = {**P.BWD_SHAPES, **P.FOLD_SHAPES}
ALL_SHAPES = {**P.FWD_SHAPES, **ALL_BWD}


def _rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def taps_of(indices, Hi, Wi):
    """max_pool2d's return_indices (flat iy * Wi + ix, NCHW) -> tap numbers r * 3 + s, NHWC."""
    B, C, Ho, Wo = indices.shape
    iy, ix = indices // Wi, indices % Wi
    oy, ox = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    r, s = iy - (2 * oy - 1), ix - (2 * ox - 1)
    assert ((r >= 0) & (r <= 2) & (s >= 0) & (s <= 2)).all()
    return nhwc(r * 3 + s).to(torch.uint8)


def _double_inputs(B, Hi, Wi, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hi, Wi, C, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) * P._signs(C).double()
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    dpool = torch.randn(B, P.out_size(Hi), P.out_size(Wi), C, generator=g, dtype=torch.float64)
    return x, gamma, beta, dpool


@pytest.mark.parametrize("name", list(ALL_SHAPES))
def test_references_equal_torch_autograd_in_double(name):
    """Plain pool and the fused stem tail, forward and backward; the two fold shapes check one image."""
    B, Hi, Wi, C = ALL_SHAPES[name]
    if name in P.FOLD_SHAPES:
        B = 1
    x, gamma, beta, dpool = _double_inputs(B, Hi, Wi, C, seed=3)
    eps = float(np.float32(R.EPS))
    # plain pool
    xt = nchw(x).requires_grad_(True)
    yt, it = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    yt.backward(nchw(dpool))
    y, idx = P.maxpool_fwd(x)
    assert torch.equal(y, nhwc(yt.detach())) and torch.equal(idx, taps_of(it, Hi, Wi))
    routed_abs = P.maxpool_bwd(dpool.abs(), idx, Hi, Wi)           # (a pixel of several windows: the order of the additions is free)
    assert ((P.maxpool_bwd(dpool, idx, Hi, Wi) - nhwc(xt.grad)).abs() <= 1e-15 * routed_abs).all()
    # fused stem tail
    xt = nchw(x).requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    if B * Hi * Wi > 1:
        bn = F.batch_norm(xt, None, None, gt, bt, True, 0.1, eps)
    else:       # torch refuses one value per channel in training mode: the same expression by hand (variance 0)
        mu = xt.mean((0, 2, 3), keepdim=True)
        bn = (xt - mu) / torch.sqrt(((xt - mu) ** 2).mean((0, 2, 3), keepdim=True) + eps) * gt.view(1, -1, 1, 1) + bt.view(1, -1, 1, 1)
    yt, it = F.max_pool2d(F.relu(bn), 3, 2, 1, return_indices=True)
    yt.backward(nchw(dpool))
    rows = x.reshape(-1, C)
    mean = rows.mean(0)
    invstd = 1.0 / torch.sqrt(((rows - mean) ** 2).mean(0) + eps)
    y, idx, pre = P.bn_relu_maxpool_fwd(x, mean, invstd, gamma, beta)
    assert _rel(y, nhwc(yt.detach())) <= 1e-12
    assert _rel(pre, nhwc(bn.detach())) <= 1e-12
    assert torch.equal(idx, taps_of(it, Hi, Wi))
    b = P.maxpool_bn_relu_bwd(dpool, idx, x, mean, invstd, gamma, beta)
    scale = max(nhwc(xt.grad).abs().max().item(), 1e-300)
    assert ((b.dx - nhwc(xt.grad)).abs().max().item() <= 1e-11 * max(scale, b.dx_mag.max().item()))
    assert (b.dgamma - gt.grad).abs().max().item() <= 1e-11 * b.A1.max().clamp_min(1.0).item()
    assert (b.dbeta - bt.grad).abs().max().item() <= 1e-11 * b.A0.max().clamp_min(1.0).item()
    assert torch.equal(b.g, P.maxpool_bwd(dpool, idx, Hi, Wi) * (pre > 0))


@pytest.mark.parametrize("name", list(P.UP_SHAPES))
@pytest.mark.parametrize("with_add", [False, True])
def test_upsample_reference_equals_torch_autograd(name, with_add):
    B, H, W, C = P.UP_SHAPES[name]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, 2 * H, 2 * W, C, generator=g, dtype=torch.float64)
    add = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) if with_add else None
    F.interpolate(x, scale_factor=2).backward(nchw(dy))
    dx, mag = P.upsample2x_bwd(dy, add)
    ref = nhwc(x.grad) + (add if with_add else 0.0)
    assert (dx - ref).abs().max().item() <= 1e-14 * mag.max().item()


@pytest.mark.parametrize("name", list(ALL_SHAPES))
def test_exact_regime_is_exact(name):
    """Integer data: the fp32 restatement of the affine step and of dx, with and without a fused multiply-add, equals the fp64 one bit for
    bit; pooled values and gradients are bf16 numbers; every partial sum stays below 2^24 units of its granule; gamma has both signs and
    a zero; ties are everywhere."""
    B, Hi, Wi, C = ALL_SHAPES[name]
    d = P.exact_inputs(B, Hi, Wi, C, seed=0)
    assert (d.gamma > 0).any() and (d.gamma < 0).any() and (d.gamma == 0).any()
    y, idx, pre = P.bn_relu_maxpool_fwd(d.x, d.mean, d.invstd, d.gamma, d.beta)
    for fused in (False, True):
        assert torch.equal(P.f32_pre_activation(d.x, d.mean, d.invstd, d.gamma, d.beta, fused).double(), pre)
    assert torch.equal(y.float().bfloat16().double(), y) and torch.equal(d.x.bfloat16().float(), d.x) and torch.equal(d.dpool.bfloat16().float(), d.dpool)
    for taps in (idx, P.random_taps(B, Hi, Wi, C, seed=0)):
        b = P.maxpool_bn_relu_bwd(d.dpool, taps, d.x, d.mean, d.invstd, d.gamma, d.beta, d.mg, d.mgx)
        for fused in (False, True):
            assert torch.equal(P.f32_dx(b.g, d.x, d.mean, d.invstd, d.gamma, d.mg, d.mgx, fused).double(), b.dx)
        # terms are multiples of 1/2 (g an integer, xhat a multiple of 1/2): any partial sum is exact while 2 * sum|term| < 2^24
        assert torch.equal((b.g * b.xhat * 2).round(), b.g * b.xhat * 2)
        assert b.A0.max().item() < 2 ** 24 and 2 * b.A1.max().item() < 2 ** 24
        assert torch.equal(b.S0.float().double(), b.S0) and torch.equal(b.S1.float().double(), b.S1)
        assert torch.equal(b.dx.float().double(), b.dx)
    if B * Hi * Wi >= 64:
        cand = P._candidates(pre.clamp_min(0.0), -1.0)
        assert ((cand == y.unsqueeze(0)).sum(0) > 1).double().mean().item() > 0.25          # ties: more than one tap holds the maximum
        assert (pre == 0).any()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", P.RANDOM_CASES + [(2, 64, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_ambiguity_share_of_every_random_case(shape, bf16):
    """The windows / elements the GPU tests leave unchecked are at most bn_ref.SKIP_CAP of each random case (same seed as the GPU file)."""
    B, Hi, Wi, C = shape
    d = P.random_inputs(B, Hi, Wi, C, seed=P.RANDOM_SEED, bf16=bf16)
    relu_unsure, tap_unsure, _ = P.ambiguity(d.x, d.mean, d.invstd, d.gamma, d.beta)
    share_relu, share_tap = relu_unsure.double().mean().item(), tap_unsure.double().mean().item()
    print(f"pool ambiguity {shape} {'bf16' if bf16 else 'f32'} relu {share_relu:.3g} tap {share_tap:.3g}")
    assert share_relu <= P.SKIP_CAP and share_tap <= P.SKIP_CAP


def test_ambiguity_rule_on_constructed_windows():
    """A 4x4 map whose window (1, 1) has all nine taps, one case per channel: an exact tie and a zero gamma are not ambiguous, a near tie
    and a window of zeros with one undecidable ReLU are."""
    C = 4
    x = torch.zeros(1, 4, 4, C)
    x[0, 1:, 1:, 0] = torch.tensor([[1.0, 5.0, 5.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])                 # exact tie of the same x
    x[0, 1:, 1:, 1] = torch.tensor([[1.0, 5.0, 5.0 + 2.0 ** -21], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])    # one ulp apart: inside the bound
    x[0, 1:, 1:, 2] = torch.arange(9.0).view(3, 3)                                                      # gamma == 0: all equal beta
    x[0, :, :, 3] = -5.0
    x[0, 2, 3, 3] = -1.0 - 2.0 ** -23                                                                   # pre = -2^-23: ReLU undecidable
    one, zero = torch.ones(C), torch.zeros(C)
    gamma, beta = torch.tensor([1.0, 1.0, 0.0, 1.0]), torch.tensor([0.25, 0.25, 0.5, 1.0])
    relu_unsure, tap_unsure, _ = P.ambiguity(x, zero, one, gamma, beta)
    assert tap_unsure[0, 1, 1].tolist() == [False, True, False, True]
    assert relu_unsure[0, 2, 3].tolist() == [False, False, False, True] and relu_unsure.sum().item() == 1
    _, idx, _ = P.bn_relu_maxpool_fwd(x, zero, one, gamma, beta)
    assert idx[0, 1, 1].tolist() == [1, 2, 0, 0]


@pytest.mark.parametrize("shape", [(4, 7, 9, 16), (4, 6, 8, 16), (8, 1, 1, 8), (8, 1, 3, 8), (8, 2, 2, 8)], ids=lambda s: "x".join(map(str, s)))
def test_random_taps_cover_every_in_bounds_tap_of_every_window_class(shape):
    B, Hi, Wi, C = shape
    taps = P.random_taps(B, Hi, Wi, C, seed=5)
    inb = P.in_bounds(Hi, Wi)
    Ho, Wo = inb.shape[1:]
    assert taps.shape == (B, Ho, Wo, C) and taps.dtype == torch.uint8
    ok = inb.permute(1, 2, 0)[None, :, :, None, :].expand(B, Ho, Wo, C, 9).gather(4, taps.long().unsqueeze(-1))
    assert ok.all(), "an out-of-bounds tap"
    cls = P.window_class(Hi, Wi)
    for k in cls.unique().tolist():
        where = cls == k
        allowed = inb[:, where][:, 0]               # the same for every window of a class
        seen = torch.zeros(9, dtype=torch.bool)
        seen[taps[:, where].reshape(-1).long().unique()] = True
        assert torch.equal(seen, allowed), f"class {k}: taps seen {seen.tolist()}, in bounds {allowed.tolist()}"
    if shape == (4, 7, 9, 16):
        assert sorted(cls.unique().tolist()) == [0, 1, 2, 4, 5, 6, 8, 9, 10]                # interior, four borders, four corners
    dy = torch.randn(B, Ho, Wo, C, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    dx = P.maxpool_bwd(dy, taps, Hi, Wi)
    assert (dx.sum((1, 2)) - dy.sum((1, 2))).abs().max().item() <= 1e-12 * dy.abs().sum((1, 2)).max().item()


def test_every_shape_reaches_the_branch_its_id_names():
    for name, (B, Hi, Wi, C) in P.FWD_SHAPES.items():
        assert (P.fwd_kernel(Wi, C, False), P.fwd_kernel(Wi, C, True)) == P.FWD_KERNELS[name], name
        assert P.fwd_kernel(Wi, C, False, pair_option=False) == P.fwd_kernel(Wi, C, True, pair_option=False) == "single"
        assert ("pair" in name.split("_")[0]) == (P.FWD_KERNELS[name][0] == "pair") or name.startswith("c12")
    assert P.out_size(3) == 2 and P.out_size(7) == 4 and P.out_size(5) == 3 and P.out_size(1) == 1
    n_threads = 3 * 3 * 4 * 16 // 2                                 # (3, 6, 8, 64): pairs of windows x float4 columns
    assert 256 < n_threads < 512 and n_threads % 256 != 0
    for name, shape in ALL_BWD.items():
        p = P.bwd_plan(*shape)
        assert p.quad == name.startswith("quad"), name
        assert (p.fold is not None) == (name in P.FOLD_SHAPES), name
    p = P.bwd_plan(*P.BWD_SHAPES["quad_one_quad_256_lanes"])
    assert (p.lanes, p.nb, p.per_lane, p.L_red) == (256, 1, 4, 260)
    p = P.bwd_plan(*P.BWD_SHAPES["quad_c1024_one_lane"])
    assert (p.lanes, p.per_lane, p.L_red) == (1, 256, 257)
    p = P.bwd_plan(*P.BWD_SHAPES["quad_two_blocks_ragged"])
    assert (p.nb, p.M % 256, p.lanes, p.per_lane) == (2, 164, 16, 16)
    p = P.bwd_plan(*P.BWD_SHAPES["pixel_odd_odd"])
    assert (p.nb, p.lanes, p.per_lane) == (1, 128, 2)
    for name, shape in P.FOLD_SHAPES.items():
        p = P.bwd_plan(*shape)
        assert p.nb > 2048 and p.fold.slab == max(16, p.nb // 128) and p.fold.rows_out == R.cdiv(p.nb, p.fold.slab) and 2 * shape[3] <= 1024
        assert p.L == P.GATHER_ADDS + p.L_red + p.fold.L
    assert P.bwd_plan(8, 256, 256, 4).fold is None                  # 2048 partial rows: the last size without the fold
    B, H, W, C = P.UP_SHAPES["two_blocks_ragged"]
    assert 256 < B * H * W * C // 4 < 512
