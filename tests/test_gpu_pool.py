"""The pooling, stem-tail, upsample and cast kernels of sd_nn.hip against the fp64 references and derived bounds of tests/pool_ref.py, per
element and per channel, at the smallest shape that reaches each branch of the host dispatch (pool_ref.FWD_SHAPES / BWD_SHAPES /
FOLD_SHAPES / UP_SHAPES name them).

Exact regime: small integers and dyadic parameters -> equality, the winning taps included (a `>=` in a tap scan, a tap number off by one, a
gradient routed through a window that does not exist, pooling x before the affine step, a truncating bf16 store all change a value).
Random regime: Gaussian activations -> identical taps outside the ambiguous windows and the bounds of pool_ref, whose docstring derives
them.  The backward takes its tap plane as an input: the reference's, then pool_ref.random_taps, which reaches every route (window, tap)
-> pixel.  Every activation, tap plane, output and workspace sits in an allocation of its own between guard regions (a finite sentinel
for inputs, NaN / a byte pattern for outputs, which also start as NaN / 0xFF): an out-of-range read changes a result, an unwritten element
fails its comparison, a write past the end changes the guard, and nothing leaves its allocation.

Each check prints `pool err/bound <case> <quantity> <ratio>`; docs/DESIGN_LOG.md holds the table of one run."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bn_ref as R
from tests import pool_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, BF16_U = P.U, P.BF16_U
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
GUARD = 2048            # elements on either side of a view
IN_SENTINEL = 1000.0    # finite (tests use no non-finite activations), a bf16 number, larger than any activation or gradient here
TAP_SENTINEL = 4        # the centre tap: in bounds for every window, so a tap read from the guard routes a gradient
OUT_PATTERN = 0xA5
_KEEP = []              # device tensors whose raw pointers go to the C ABI outlive the launch: released after the test's last synchronisation
_GUARDS = []


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _GUARDS.clear()
    _KEEP.clear()


class Guarded:
    """`n` elements at element `offset` (+ GUARD) of a larger allocation, sentinel before and after."""

    def __init__(self, n, dtype, fill, sentinel, offset=0):
        self.n, self.lo, self.sentinel = n, GUARD + offset, sentinel
        self.buf = torch.full((self.lo + n + GUARD,), sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[self.lo:self.lo + n]
        if fill is not None:
            self.view.fill_(fill)
        _KEEP.append(self.buf)
        _GUARDS.append(self)

    def intact(self):
        g = torch.cat([self.buf[:self.lo], self.buf[self.lo + self.n:]])
        return bool(torch.isnan(g).all()) if isinstance(self.sentinel, float) and np.isnan(self.sentinel) else bool((g == self.sentinel).all())


def check_guards(case):
    torch.cuda.synchronize()
    for i, g in enumerate(_GUARDS):
        assert g.intact(), f"{case}: guard region of allocation {i} ({g.buf.dtype}, {g.n} elements) was written"
    _GUARDS.clear()


def inp(t, dtype, offset=0):
    """Host tensor -> device view of the same shape inside a guarded allocation."""
    sentinel = TAP_SENTINEL if dtype == U8 else IN_SENTINEL
    g = Guarded(t.numel(), dtype, None, sentinel, offset)
    g.view.copy_(t.reshape(-1).to(DEV))
    return g.view.view(t.shape)


def out(shape, dtype, offset=0):
    n = int(np.prod(shape))
    if dtype == U8:
        return Guarded(n, U8, 0xFF, OUT_PATTERN, offset).view.view(shape)
    return Guarded(n, dtype, float("nan"), float("nan"), offset).view.view(shape)


def workspace(M, Cc):
    """Exactly sd_col_reduce_workspace_bytes(M, C) usable bytes of 0xFF (NaN as floats) before the guard."""
    from structuredetector_amd import _lib as L
    return Guarded(L.lib().sd_col_reduce_workspace_bytes(M, Cc), U8, 0xFF, OUT_PATTERN).view


def params(d):
    return SimpleNamespace(**{k: inp(getattr(d, k).float(), F32) for k in ("mean", "invstd", "gamma", "beta")})


def ptr(t):
    return 0 if t is None else t.data_ptr()


def report(case, what, ratio):
    print(f"pool err/bound {case} {what} {ratio:.4g}")


def check_bound(case, what, got, ref, bound, skip=None):
    """|got - ref| <= bound elementwise (fp64 on the host); NaN fails; `skip` marks elements left unchecked."""
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    err = (got.detach().cpu().double() - ref).abs()
    bad = ~(err <= bound)
    if skip is not None:
        bad &= ~skip
        err = err.masked_fill(skip, 0.0)
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    report(case, what, ratio)
    assert not bad.any(), f"{case} {what}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err/bound {ratio:.4g}"


def check_same(case, what, got, ref, skip=None):
    """Bitwise-equal values (NaN never equal): `ref` a host tensor of values the output type represents exactly."""
    g, r = got.detach().cpu(), ref.to(got.dtype) if ref.dtype == U8 else ref.float().to(got.dtype)
    assert g.shape == r.shape, f"{case} {what}: shape"
    bad = ~(g == r)
    if skip is not None:
        bad &= ~skip
    report(case, what, 0.0 if not bad.any() else float("inf"))
    assert not bad.any(), f"{case} {what}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[0].tolist()}"


def f32_add(prior, total):
    """prior + (float)total as the finish kernels accumulate: one fp32 addition."""
    return torch.from_numpy(prior.numpy().astype(np.float32) + total.numpy().astype(np.float32))


def lib_call(name, *args):
    from structuredetector_amd import _lib as L
    L.check(getattr(L.lib(), name)(*args, L.stream()), name)


def set_pair(v):
    from structuredetector_amd import _lib as L
    L.check(L.lib().sd_set_option(b"pool_fwd_pair", v))


def tag(dtype):
    return "bf16" if dtype == BF16 else "f32"


def rounded(dtype):
    return (lambda t: t.float().bfloat16().double()) if dtype == BF16 else (lambda t: t.float().double())


def store(dtype, ref):
    return BF16_U * ref.abs() if dtype == BF16 else torch.zeros_like(ref)


def inputs(shape, exact, bf16):
    return P.exact_inputs(*shape, seed=0) if exact else P.random_inputs(*shape, seed=P.RANDOM_SEED, bf16=bf16)


SHAPE_IDS = lambda s: "x".join(map(str, s))
POOL_SHAPES = sorted(set(P.FWD_SHAPES.values()) | set(P.BWD_SHAPES.values()))
REGIMES = [pytest.param(True, id="exact"), pytest.param(False, id="random")]
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]


# ---- plain pool ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=SHAPE_IDS)
def test_plain_maxpool(shape, exact):
    """sd_maxpool3x3s2_fwd / _fwd_bf16 / _bwd: a maximum is exact, so y and idx equal the reference in both regimes, on fp32 and on
    bf16-rounded values; the backward from the reference's taps and from random_taps (equal / 4u * sum|dy routed|)."""
    B, Hi, Wi, Cc = shape
    Ho, Wo = P.out_size(Hi), P.out_size(Wi)
    case = f"plain-{SHAPE_IDS(shape)}-{'exact' if exact else 'random'}"
    for bf in (False, True):
        d = inputs(shape, exact, bf)
        yref, iref = P.maxpool_fwd(d.x)
        y, idx = out((B, Ho, Wo, Cc), F32), out((B, Ho, Wo, Cc), U8)
        lib_call("sd_maxpool3x3s2_fwd", ptr(inp(d.x, F32)), ptr(y), ptr(idx), B, Hi, Wi, Cc)
        check_same(case, f"y_{tag(BF16 if bf else F32)}_values", y, yref)
        check_same(case, f"idx_{tag(BF16 if bf else F32)}_values", idx, iref)
        if bf and Cc % 8 == 0:
            y16 = out((B, Ho, Wo, Cc), BF16)
            lib_call("sd_maxpool3x3s2_fwd_bf16", ptr(inp(d.x, BF16)), ptr(y16), B, Hi, Wi, Cc)
            check_same(case, "y_bf16_kernel", y16, yref)
    d = inputs(shape, exact, False)
    _, iref = P.maxpool_fwd(d.x)
    for what, taps in (("ref_taps", iref), ("random_taps", P.random_taps(*shape, seed=2))):
        dx = out(shape, F32)
        lib_call("sd_maxpool3x3s2_bwd", ptr(inp(d.dpool, F32)), ptr(inp(taps, U8)), ptr(dx), B, Hi, Wi, Cc)
        ref = P.maxpool_bwd(d.dpool, taps, Hi, Wi)
        if exact:
            check_same(case, f"dx_{what}", dx, ref)
        else:
            check_bound(case, f"dx_{what}", dx, ref, 4 * U * P.maxpool_bwd(d.dpool.abs(), taps, Hi, Wi))
    check_guards(case)


# ---- fused forward ------------------------------------------------------------------------------------------------------------------
def run_fused_fwd(case, d, shape, dtype, exact, offset=0):
    """sd_bn_relu_maxpool_fwd[_bf16] with the pair option on and off against the reference; returns (y, idx) of both runs."""
    B, Hi, Wi, Cc = shape
    Ho, Wo = P.out_size(Hi), P.out_size(Wi)
    name = "sd_bn_relu_maxpool_fwd" + ("_bf16" if dtype == BF16 else "")
    yref, iref, pre = P.bn_relu_maxpool_fwd(d.x, d.mean, d.invstd, d.gamma, d.beta)
    if not exact:
        _, tap_unsure, b = P.ambiguity(d.x, d.mean, d.invstd, d.gamma, d.beta)
        assert tap_unsure.double().mean().item() <= P.SKIP_CAP
        bound = P.tap_gather(b, iref) + store(dtype, yref)
    x, pp = inp(d.x, dtype, offset), params(d)
    assert x.data_ptr() % 16 == (8 if offset else 0)
    results = []
    try:
        for pair in (1, 0):
            set_pair(pair)
            y, idx = out((B, Ho, Wo, Cc), dtype), out((B, Ho, Wo, Cc), U8)
            lib_call(name, ptr(x), B, Hi, Wi, Cc, ptr(pp.mean), ptr(pp.invstd), ptr(pp.gamma), ptr(pp.beta), ptr(y), ptr(idx))
            what = f"pair{pair}"
            if exact:
                check_same(case, f"idx_{what}", idx, iref)
                check_same(case, f"y_{what}", y, rounded(dtype)(yref))
            else:
                check_same(case, f"idx_{what}", idx, iref, skip=tap_unsure)
                check_bound(case, f"y_{what}", y, yref, bound, skip=tap_unsure)
            results.append((y, idx))
    finally:
        set_pair(1)
    (y1, i1), (y0, i0) = results
    assert torch.equal(y1, y0) and torch.equal(i1, i0), f"{case}: two windows per thread differ from one window per thread"
    check_guards(case)
    return results


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("name", list(P.FWD_SHAPES))
def test_fused_forward(name, exact, dtype):
    """BatchNorm -> ReLU -> MaxPool forward at the shapes of pool_ref.FWD_SHAPES, fp32 and bf16, both kernels of the dispatch."""
    shape = P.FWD_SHAPES[name]
    bf = dtype == BF16
    assert P.fwd_kernel(shape[2], shape[3], bf) == P.FWD_KERNELS[name][1 if bf else 0]
    assert P.fwd_kernel(shape[2], shape[3], bf, pair_option=False) == "single"
    run_fused_fwd(f"fwd-{name}-{'exact' if exact else 'random'}-{tag(dtype)}", inputs(shape, exact, bf), shape, dtype, exact)


@pytest.mark.parametrize("exact", REGIMES)
def test_fused_forward_bf16_view_8_bytes_into_its_allocation(exact):
    """A bf16 x that is 8-byte but not 16-byte aligned reaches the single-window kernel whatever the option says: the same results."""
    shape = P.FWD_SHAPES["pair_two_blocks_ragged"]
    d = inputs(shape, exact, True)
    case = f"fwd-offset8-{'exact' if exact else 'random'}-bf16"
    (y_off, i_off), _ = run_fused_fwd(case, d, shape, BF16, exact, offset=4)
    (y_al, i_al), _ = run_fused_fwd(case + "-aligned", d, shape, BF16, exact)
    assert torch.equal(y_off, y_al) and torch.equal(i_off, i_al)


# ---- fused backward -----------------------------------------------------------------------------------------------------------------
KINDS = {  # name -> (suffix of the whole call, of the reduce half, of the apply half, input type, dx type)
    "f32": ("", "", "", F32, F32),
    "bf16": ("_bf16", "_bf16", "_bf16", BF16, F32),
    "bf16_dx16": ("_bf16_dx16", "_bf16", "_bf16_dx16", BF16, BF16),
}


def bwd_args(dpool, idx, x, shape, pp):
    B, Hi, Wi, Cc = shape
    return (ptr(dpool), ptr(idx), ptr(x), B, Hi, Wi, Cc, ptr(pp.mean), ptr(pp.invstd), ptr(pp.gamma), ptr(pp.beta))


def run_fused_bwd(case, shape, exact):
    B, Hi, Wi, Cc = shape
    plan = P.bwd_plan(*shape)
    n = plan.M
    kinds = ["f32", "bf16", "bf16_dx16"] if plan.quad else ["f32"]
    for taps_name in ("ref_taps", "random_taps"):
        refs = {}
        for kind in kinds:
            whole, red, app, in_t, dx_t = KINDS[kind]
            bf = in_t == BF16
            key = bf and not exact
            if key not in refs:
                d = inputs(shape, exact, bf)
                taps = P.bn_relu_maxpool_fwd(d.x, d.mean, d.invstd, d.gamma, d.beta)[1] if taps_name == "ref_taps" else P.random_taps(*shape, seed=7)
                ref = P.maxpool_bn_relu_bwd(d.dpool, taps, d.x, d.mean, d.invstd, d.gamma, d.beta, *((d.mg, d.mgx) if exact else ()))
                refs[key] = (d, taps, ref)
            d, taps, ref = refs[key]
            c = f"{case}-{kind}-{taps_name}"
            dpool, idx, x, pp = inp(d.dpool, in_t), inp(taps, U8), inp(d.x, in_t), params(d)
            args = bwd_args(dpool, idx, x, shape, pp)
            if exact:
                prior0, prior1 = d.prior0.float(), d.prior1.float()
                dg0, db0, dg1, db1 = out((Cc,), F32), out((Cc,), F32), inp(prior0, F32), inp(prior1, F32)
                sums, ws = out((2 * Cc + 1,), torch.float64), workspace(n, Cc)
                lib_call("sd_maxpool_bn_relu_bwd_reduce" + red, *args, ptr(dg0), ptr(db0), 0, ptr(sums), ptr(ws), ws.numel())
                lib_call("sd_maxpool_bn_relu_bwd_reduce" + red, *args, ptr(dg1), ptr(db1), 1, ptr(sums), ptr(ws), ws.numel())
                sh = sums.cpu()
                assert sh[2 * Cc].item() == n, f"{c}: n"
                assert max(ref.S0.abs().max().item(), ref.S1.abs().max().item()) < 2 ** 24
                check_same(c, "sum_g", sh[:Cc], ref.S0)
                check_same(c, "sum_gxhat", sh[Cc:2 * Cc], ref.S1)
                check_same(c, "dbeta", db0, ref.S0)
                check_same(c, "dgamma", dg0, ref.S1)
                check_same(c, "dbeta_accumulate", db1, f32_add(prior1, ref.S0))
                check_same(c, "dgamma_accumulate", dg1, f32_add(prior0, ref.S1))
                dx = out(shape, dx_t)
                lib_call("sd_maxpool_bn_relu_bwd_apply" + app, *args, ptr(inp(torch.cat([d.mg, d.mgx]), F32)), ptr(dx))
                check_same(c, "dx", dx, rounded(dx_t)(ref.dx))
            else:
                relu_unsure, _, _ = P.ambiguity(d.x, d.mean, d.invstd, d.gamma, d.beta)
                assert relu_unsure.double().mean().item() <= P.SKIP_CAP
                lost = ref.routed_abs * relu_unsure            # an undecidable ReLU may add or drop its whole term
                b0 = R.sum_bound(plan.L, ref.A0) + lost.sum((0, 1, 2))
                b1 = R.sum_bound(plan.L, ref.A1) + (lost * ref.xhat.abs()).sum((0, 1, 2))
                dx, dg, db, ws = out(shape, dx_t), out((Cc,), F32), out((Cc,), F32), workspace(n, Cc)
                lib_call("sd_maxpool_bn_relu_bwd" + whole, *args, ptr(dx), ptr(dg), ptr(db), 0, ptr(ws), ws.numel())
                check_bound(c, "dbeta", db, ref.dbeta, b0)
                check_bound(c, "dgamma", dg, ref.dgamma, b1)
                e_mg, e_mgx = b0 / n + 2 * U * ref.mg.abs(), b1 / n + 2 * U * ref.mgx.abs()
                bound = 8 * U * ref.dx_mag + ref.k.abs() * (e_mg + ref.xhat.abs() * e_mgx) + store(dx_t, ref.dx)
                check_bound(c, "dx", dx, ref.dx, bound, skip=relu_unsure)
            check_guards(c)


@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("name", list(P.BWD_SHAPES))
def test_fused_backward(name, exact):
    """MaxPool -> ReLU -> BatchNorm backward at the shapes of pool_ref.BWD_SHAPES: fp32, bf16 in / fp32 dx, bf16 in / bf16 dx (the bf16
    forms on even maps).  Exact: the split forms of synchronized BatchNorm (reduce with fp64 sums, accumulate 0 and 1; apply from dyadic
    means).  Random: the whole call against the fp64 reference inside the derived bounds."""
    shape = P.BWD_SHAPES[name]
    assert P.bwd_plan(*shape).quad == name.startswith("quad") and P.bwd_plan(*shape).fold is None
    run_fused_bwd(f"bwd-{name}-{'exact' if exact else 'random'}", shape, exact)


@pytest.mark.parametrize("name", list(P.FOLD_SHAPES))
def test_fused_backward_rows_fold(name):
    """More than 2048 partial rows: k_rows_fold between the reduction and the finish.  Exact regime only: integer equality."""
    shape = P.FOLD_SHAPES[name]
    plan = P.bwd_plan(*shape)
    assert plan.nb == 2304 and plan.fold is not None and plan.quad == name.startswith("quad")
    run_fused_bwd(f"bwd-{name}-exact", shape, True)


def test_bf16_backward_refuses_odd_maps():
    """The bf16 forms have no pixel kernel: odd Hi or Wi returns an error that names the function and writes nothing."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    for shape in ((1, 3, 4, 8), (1, 4, 3, 8)):
        B, Hi, Wi, Cc = shape
        d = P.exact_inputs(*shape)
        taps = P.random_taps(*shape)
        dpool, idx, x, pp = inp(d.dpool, BF16), inp(taps, U8), inp(d.x, BF16), params(d)
        args = bwd_args(dpool, idx, x, shape, pp)
        means = inp(torch.cat([d.mg, d.mgx]), F32)
        for name, dx_t in (("sd_maxpool_bn_relu_bwd_bf16", F32), ("sd_maxpool_bn_relu_bwd_bf16_dx16", BF16)):
            dx, dg, db, ws = out(shape, dx_t), out((Cc,), F32), out((Cc,), F32), workspace(B * Hi * Wi, Cc)
            rc = getattr(lib, name)(*args, ptr(dx), ptr(dg), ptr(db), 0, ptr(ws), ws.numel(), L.stream())
            assert rc != 0 and name in lib.sd_last_error().decode(), name
            torch.cuda.synchronize()
            assert torch.isnan(dx).all() and torch.isnan(dg).all() and torch.isnan(db).all() and (ws == 0xFF).all(), name
        name = "sd_maxpool_bn_relu_bwd_reduce_bf16"
        dg, db, sums, ws = out((Cc,), F32), out((Cc,), F32), out((2 * Cc + 1,), torch.float64), workspace(B * Hi * Wi, Cc)
        rc = getattr(lib, name)(*args, ptr(dg), ptr(db), 0, ptr(sums), ptr(ws), ws.numel(), L.stream())
        assert rc != 0 and name in lib.sd_last_error().decode(), name
        torch.cuda.synchronize()
        assert torch.isnan(dg).all() and torch.isnan(db).all() and torch.isnan(sums).all() and (ws == 0xFF).all(), name
        for name, dx_t in (("sd_maxpool_bn_relu_bwd_apply_bf16", F32), ("sd_maxpool_bn_relu_bwd_apply_bf16_dx16", BF16)):
            dx = out(shape, dx_t)
            rc = getattr(lib, name)(*args, ptr(means), ptr(dx), L.stream())
            assert rc != 0 and name in lib.sd_last_error().decode(), name
            torch.cuda.synchronize()
            assert torch.isnan(dx).all(), name
        check_guards(f"refuse-{SHAPE_IDS(shape)}")


# ---- upsample backward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("name", list(P.UP_SHAPES))
def test_upsample2x_backward(name, exact, dtype):
    """sd_upsample2x_bwd[_bf16]: the 2x2 block sums with `add` null and non-null (equal / 5u * sum|terms|, + one bf16 rounding)."""
    B, H, W, Cc = P.UP_SHAPES[name]
    g = torch.Generator().manual_seed(11)
    if exact:
        dy, add = torch.randint(-4, 5, (B, 2 * H, 2 * W, Cc), generator=g).float(), torch.randint(-4, 5, (B, H, W, Cc), generator=g).float()
    else:
        scale = 2.0 ** ((torch.arange(Cc) % 5) - 2).float()
        dy, add = torch.randn(B, 2 * H, 2 * W, Cc, generator=g) * scale, torch.randn(B, H, W, Cc, generator=g) * scale
        if dtype == BF16:
            dy, add = dy.bfloat16().float(), add.bfloat16().float()
    fn = "sd_upsample2x_bwd" + ("_bf16" if dtype == BF16 else "")
    dyd = inp(dy, dtype)
    for with_add in (False, True):
        case = f"up-{name}-{'exact' if exact else 'random'}-{tag(dtype)}"
        what = "dx_add" if with_add else "dx"
        dx = out((B, H, W, Cc), dtype)
        lib_call(fn, ptr(dyd), ptr(inp(add, dtype)) if with_add else 0, ptr(dx), B, H, W, Cc)
        ref, mag = P.upsample2x_bwd(dy, add if with_add else None)
        if exact:
            check_same(case, what, dx, rounded(dtype)(ref))
        else:
            check_bound(case, what, dx, ref, 5 * U * mag + store(dtype, ref))
    check_guards(case)


# ---- casts --------------------------------------------------------------------------------------------------------------------------
def _cast_table():
    """fp32 bit patterns around every rounding decision of the cast to bf16."""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x0080, 0x0001, 0x0000, 0x7F7E, 0x7F7F):      # even / odd mantissa, normal, smallest normal, denormals, the largest
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):                   # exact, just above, below / at / above halfway, just below the next
            for sign in (0, 0x80000000):
                bits.append(sign | (hi << 16) | lo)
    bits += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF]          # +-0, +-inf, NaNs
    while len(bits) % 4:
        bits.append(0)
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def _cast_to_bf16(x):
    y = out((x.numel(),), BF16)
    lib_call("sd_cast_f32_to_bf16", ptr(inp(x, F32)), ptr(y), x.numel())
    return y


def test_cast_to_bf16_rounds_to_nearest_even_on_the_special_values():
    """sd_cast_f32_to_bf16 = torch.Tensor.bfloat16() bit for bit on halfway cases around even and odd mantissas, +-0, denormals, both sides
    of the overflow to inf, +-inf; NaN stays NaN (payload not compared)."""
    x = _cast_table()
    assert x.isnan().sum().item() == 4 and x.isinf().sum().item() == 2
    ref = x.bfloat16()
    got = _cast_to_bf16(x).cpu()
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan)
    gb, rb = got.view(torch.int16), ref.view(torch.int16)
    bad = (gb != rb) & ~nan
    assert not bad.any(), [(hex(v), hex(a & 0xFFFF), hex(b & 0xFFFF)) for v, a, b in
                           zip(x.view(torch.int32)[bad].tolist(), gb[bad].tolist(), rb[bad].tolist())]
    assert ref.isinf().sum().item() > 2 and (ref.float() != x)[~nan].any()            # the table overflows and rounds
    report("cast-table", "f32_to_bf16", 0.0)
    check_guards("cast-table")


@pytest.mark.parametrize("n", [4, 4 * (4096 * 256) + 4 * 37], ids=["one_thread", "second_trip_ragged"])
def test_casts_at_the_grid_stride_sizes(n):
    """Gaussian data at n = 4 and at a size where one thread takes a second trip of the grid-stride loop with a ragged end: to bf16 as
    torch rounds, back to fp32 exactly."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    y = _cast_to_bf16(x)
    ref = x.bfloat16()
    assert torch.equal(y.cpu().view(torch.int16), ref.view(torch.int16))
    back = out((n,), F32)
    lib_call("sd_cast_bf16_to_f32", ptr(y), ptr(back), n)
    assert torch.equal(back.cpu(), ref.float())
    report(f"cast-n{n}", "round_trip", 0.0)
    check_guards(f"cast-n{n}")


def test_workspace_restatement_matches_the_library():
    """The pool reduction writes cdiv(M, 256) partial rows, the two means and the fold's slab sums into a workspace sized by
    sd_col_reduce_workspace_bytes(M, C): what bwd_plan restates fits into it at every shape used here."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    for shape in list(P.BWD_SHAPES.values()) + list(P.FOLD_SHAPES.values()):
        p = P.bwd_plan(*shape)
        Cc = shape[3]
        need = (p.nb + (p.fold.rows_out if p.fold else 0)) * 2 * Cc * 4 + 2 * Cc * 4
        assert need <= lib.sd_col_reduce_workspace_bytes(p.M, Cc), shape
        assert lib.sd_bn_finalize_scratch_rows(p.nb) == R.fold_rows(p.nb)
