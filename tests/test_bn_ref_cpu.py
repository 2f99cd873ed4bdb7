"""CPU checks of tests/bn_ref.py: the fp64 reference against torch.nn.BatchNorm2d in double, the derived error bounds against fp32
emulations of what the kernels compute, the preconditions of the exact-sum regime, and that every shape reaches the branch its id names."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R

U = R.U


def _rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_reference_equals_torch_batchnorm_in_double(relu, with_res):
    B, C, H, W = 3, 8, 5, 7
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    res = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).requires_grad_(True) if with_res else None
    dy = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(C, eps=float(np.float32(R.EPS)), momentum=R.MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5); bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=torch.float64)); bn.running_var.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    y = bn(x)
    if with_res:
        y = y + res
    if relu:
        y = F.relu(y)
    y.backward(dy)
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, C)
    M = B * H * W
    ref = R.bn_train_reference(rows(x), bn.weight.detach(), bn.bias.detach(), rows(dy), rows(res) if with_res else None, relu, eps=R.EPS)
    S0, S1, _ = R.stats_sums(rows(x))
    _, _, rm, rv = R.stats_tail(S0, S1, M, R.EPS, R.MOMENTUM, rm0, rv0)
    assert _rel(ref.y, rows(y)) <= 1e-12
    assert _rel(rm, bn.running_mean) <= 1e-12 and _rel(rv, bn.running_var) <= 1e-12
    assert _rel(ref.dx, rows(x.grad)) <= 1e-12
    assert _rel(ref.dgamma, bn.weight.grad) <= 1e-12 and _rel(ref.dbeta, bn.bias.grad) <= 1e-12
    if with_res:
        assert _rel(ref.g, rows(res.grad)) <= 1e-12


def test_unbiased_variance_falls_back_to_biased_for_one_row():
    x = torch.tensor([[3.0, -1.5, 0.0, 2.0]])
    S0, S1, _ = R.stats_sums(x)
    mean, invstd, rm, rv = R.stats_tail(S0, S1, 1, R.EPS, 0.5, torch.zeros(4), torch.ones(4))
    assert torch.equal(mean, x[0].double()) and torch.allclose(invstd, torch.full((4,), float(np.float32(R.EPS)) ** -0.5, dtype=torch.float64))
    assert torch.equal(rv, torch.full((4,), 0.5, dtype=torch.float64)) and torch.equal(rm, 0.5 * x[0].double())


def test_mask_bytes_round_trip():
    bits = torch.rand(6, 8, generator=torch.Generator().manual_seed(1)) > 0.5
    m = R.pack_mask(bits)
    assert m.shape == (12,) and torch.equal(R.unpack_mask(m, 6, 8), bits)
    assert R.pack_mask(torch.tensor([[True, False, False, True]])).item() == 9


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_each_shape_reaches_the_branch_its_id_names(name):
    M, C = R.SHAPES[name]
    p = R.plan(M, C)
    want = {"one_block_rows_lt_lanes": lambda: p.nb == 1 and M < p.lanes,
            "c4_256_lanes_tail_block": lambda: p.lanes == 256 and p.rpb == 16 and M % p.rpb == 5,
            "c1024_one_lane_f32_grid_stride": lambda: p.lanes == 1 and p.nb == 257 and R.grid_stride_iterations(M, C) == 2,
            "rpb32_second_trip_no_fold": lambda: p.rpb == 32 and p.nb == 1250 and p.trips == 3 and p.fold is None and C % 8 == 0,
            "rpb64_ragged_f32_grid_stride": lambda: p.rpb == 64 and M % 64 and R.grid_stride_iterations(M, C) == 2 and R.grid_stride_iterations(M, C, 8) == 1,
            "rpb128_bf16x8_grid_stride": lambda: p.rpb == 128 and R.grid_stride_iterations(M, C, 8) == 2,
            "rpb256_rows_fold_ragged_slab": lambda: p.rpb == 256 and p.nb == 2110 and p.fold and p.fold.slab < p.fold.lanes and p.nb % p.fold.slab}[name]
    assert want(), vars(p)
    assert M * C * 4 <= 36 << 20


def test_row_cases_reach_their_branches():
    f = {n: R.fold_plan(rows, C) for n, (rows, C) in R.ROW_CASES.items()}
    assert f["one_row"] is None and f["ragged_trip_65"] is None and f["last_without_fold_2048"] is None
    a = f["fold_one_lane_one_row_slab_2049"]
    assert a.lanes == 1 and a.slab == 16 and a.rows_out == 129 and 2049 % 16 == 1
    b = f["conv_epilogue_max_8192"]
    assert b.slab == 64 and b.rows_out == 128 and b.lanes == 8
    assert f["wide_no_fold_six_trips_3000"] is None and R.fold_rows(3000) > 0 and R.cdiv(3000, 512) == 6
    assert R.fold_plan(2049, 512, scratch=False) is None


@pytest.mark.parametrize("ratio", [0.0, 4.0, 32.0])
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_emulated_summation_order_stays_inside_the_sum_bound(name, ratio):
    """Per-lane sequential fp32 sums, lane sums, the fp32 fold, fp64 across blocks: inside (L + 2) u sum|t| for sum x and sum x^2, and the
    statistics that follow inside the propagated invstd bound."""
    M, C = R.SHAPES[name]
    d = R.random_inputs(M, C, seed=3, ratio=ratio)
    p = R.plan(M, C)
    x = d.x.numpy()
    S0, S1, A0 = R.stats_sums(d.x)
    e0 = torch.from_numpy(R.emulate_column_sums(x, C))
    e1 = torch.from_numpy(R.emulate_column_sums(x * x, C))
    b0, b1 = R.sum_bound(p.L, A0), R.sum_bound(p.L, S1)
    r0, r1 = ((e0 - S0).abs() / b0).max().item(), ((e1 - S1).abs() / b1).max().item()
    _, inv, _, _ = R.stats_tail(S0, S1, M, R.EPS)
    _, inv_e, _, _ = R.stats_tail(e0, e1, M, R.EPS)
    bi = R.invstd_bound(S0, S1, b0, b1, M, R.EPS)
    ri = ((inv_e - inv).abs() / bi).max().item()
    print(f"emulation {name} |mu|/sigma={ratio}: L={p.L} err/bound S0 {r0:.4f} S1 {r1:.4f} invstd {ri:.4f} (bound rel {(bi / inv).max().item():.2e})")
    assert r0 <= 1 and r1 <= 1 and ri <= 1


@pytest.mark.parametrize("ratio", [None, 0.0, 4.0, 32.0])
def test_fp32_formulas_stay_inside_their_bounds_and_few_relu_decisions_are_skipped(ratio):
    M, C = 20000, 64
    d = R.random_inputs(M, C, seed=7, ratio=ratio)
    f = np.float32
    x, mu, is_, ga, be, res, dy = (t.numpy() for t in (d.x, d.mean, d.invstd, d.gamma, d.beta, d.res, d.dy))
    pre, mag = R.pre_activation(d.x, d.mean, d.invstd, d.gamma, d.beta, d.res)
    for y32 in (((x - mu) * is_ * ga + be) + res,                                                   # separate multiply and add
                ((((x - mu) * is_).astype(np.float64) * ga + be).astype(f) + res)):                 # fused multiply-add
        r = ((torch.from_numpy(y32).double() - pre).abs() / (U * mag)).max().item()
        assert r <= 6, r
    pre0, mag0 = R.pre_activation(d.x, d.mean, d.invstd, d.gamma, d.beta)
    skipped = (pre0.abs() <= 6 * U * mag0).double().mean().item()
    assert skipped < R.SKIP_CAP and (pre.abs() <= 6 * U * mag).double().mean().item() < R.SKIP_CAP
    g = d.dy.double() * (pre0 > 0)
    xhat, T0, T1, _, _ = R.bwd_terms(g, d.x, d.mean, d.invstd)
    mg, mgx = (T0 / M).float(), (T1 / M).float()
    dx, magd = R.bwd_apply(g, xhat, d.gamma, d.invstd, mg, mgx)
    g32 = g.float().numpy()
    dx32 = ga * is_ * (g32 - mg.numpy() - (x - mu) * is_ * mgx.numpy())
    r = ((torch.from_numpy(dx32).double() - dx).abs() / (U * magd).clamp_min(1e-300)).max().item()
    assert r <= 8, r


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_exact_inputs_keep_every_sum_exact(name):
    """Every operand, term and total of the exact regime is an fp32 number, every fp32-stage partial sum (one block, one fold slab) stays
    below 2^24 units of its grid, and the inputs hold what each sharp check needs: zero pre-activations, zeros in y, a non-zero first
    block (the `row < nblocks` guard re-reads row 0), a ragged tail."""
    M, C = R.SHAPES[name]
    d = R.exact_inputs(M, C)
    p = R.plan(M, C)
    for t in (d.x, d.dy, d.res, d.y1, d.mean, d.invstd, d.gamma, d.beta, d.mg, d.mgx):
        assert torch.equal(t.bfloat16().float(), t)                          # exact in bf16, hence in fp32
    pre, _ = R.pre_activation(d.x, d.mean, d.invstd, d.gamma, d.beta)
    assert torch.equal(pre.float().double(), pre) and torch.equal(pre.bfloat16().double(), pre)
    zeros = (pre == 0)
    assert zeros.any() and ((d.y1 == 0) & (d.dy != 0)).any() and (zeros & (d.dy != 0)).any()
    prer, _ = R.pre_activation(d.x, d.mean, d.invstd, d.gamma, d.beta, d.res)
    assert torch.equal(prer.bfloat16().double(), prer) and (prer == 0).any()
    stage_rows = p.rpb * (p.fold.slab if p.fold else 1)                       # rows behind one fp32 accumulation
    for g in (d.dy.double(), d.dy.double() * (d.y1 > 0), d.dy.double() * (pre > 0), d.dy.double() * R.unpack_mask(d.maskbytes, M, C)):
        xhat, T0, T1, A0, A1 = R.bwd_terms(g, d.x, d.mean, d.invstd)
        t1 = g * xhat
        assert torch.equal(t1 * 2, (t1 * 2).round())                          # multiples of 1/2 ...
        assert t1.abs().max().item() * 2 * stage_rows < 2 ** 24               # ... so 2^23 bounds the exact fp32 range
        for T in (T0, T1):
            assert T.abs().max().item() < 2 ** 24 and torch.equal(T.float().double(), T)
        dx, _ = R.bwd_apply(g, xhat, d.gamma, d.invstd, d.mg, d.mgx)
        assert torch.equal(dx.float().double(), dx)
    S0, S1, A0 = R.stats_sums(d.x)
    assert 9 * stage_rows < 2 ** 24 and max(S0.abs().max().item(), S1.max().item()) < 2 ** 24
    assert (d.x[:min(p.rpb, M)].sum(0) != 0).any() and (d.dy[:min(p.rpb, M)].sum(0) != 0).any()
