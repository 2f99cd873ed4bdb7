"""The BatchNorm passes and the column-sum machinery of sd_nn.hip against the fp64 references and derived bounds of tests/bn_ref.py, per
channel and per element, at the smallest shape that reaches each branch of the host dispatch (bn_ref.SHAPES / ROW_CASES name them).

Exact regime: small integers -> equality with the integer sums and the exact elementwise results (a dropped, doubled or misplaced row,
a `>=` in the ReLU decision, a truncating bf16 store all change a value).  Random regime: Gaussian activations with per-channel scale
and offset -> the bounds of bn_ref, whose docstring derives them.  Every activation tensor is followed by 256 guard rows of a non-zero
sentinel inside its own allocation, every output and workspace starts as NaN: a read past the last row changes a sum, an unwritten
element fails its comparison, and neither leaves the allocation.

Each check prints `bn err/bound <case> <quantity> <ratio>`; docs/DESIGN_LOG.md holds the table of one run."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
F32, BF16 = torch.float32, torch.bfloat16
GUARD_ROWS = 256
_KEEP = []   # device tensors whose raw pointers go to the C ABI outlive the launch: released after the test's last synchronisation


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def keep(t):
    _KEEP.append(t)
    return t


def dev(t, dtype=None):
    t = t.to(DEV)
    return keep((t if dtype is None else t.to(dtype)).contiguous())


def nan_like_empty(n, dtype):
    if dtype == torch.uint8:
        return keep(torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV))
    return keep(torch.full((n,), float("nan"), dtype=dtype, device=DEV))


def act(t, dtype, offset=0, sentinel=7.0):
    """[M][C] host tensor -> device view at element `offset` of a larger allocation, followed by guard rows of `sentinel`."""
    M, Cc = t.shape
    buf = keep(torch.full((offset + (M + GUARD_ROWS) * Cc,), sentinel, dtype=dtype, device=DEV))
    view = buf[offset:offset + M * Cc].view(M, Cc)
    view.copy_(t.to(DEV))
    return view


def out_act(M, Cc, dtype, offset=0):
    buf = nan_like_empty(offset + M * Cc, dtype)
    return buf[offset:offset + M * Cc].view(M, Cc)


def ptr(t):
    return 0 if t is None else t.data_ptr()


def report(case, what, ratio):
    print(f"bn err/bound {case} {what} {ratio:.4g}")


def check_bound(case, what, got, ref, bound, skip=None):
    """|got - ref| <= bound elementwise (fp64 on the host); NaN fails; `skip` marks elements left unchecked."""
    err = (got.detach().cpu().double() - ref).abs()
    bad = ~(err <= bound)
    if skip is not None:
        bad &= ~skip
        err = err.masked_fill(skip, 0.0)
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    report(case, what, ratio)
    assert not bad.any(), f"{case} {what}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err/bound {ratio:.4g}"


def check_tail(case, what, got, ref, extra=0.0):
    """An fp64 expression rounded once to fp32: one ulp (2u relative)."""
    check_bound(case, what, got, ref, 2 * U * ref.abs() + extra)


def same(got, ref, dtype=None):
    """Bitwise-equal values (NaN never equal): `ref` is a host fp64 tensor of exactly representable values, or a device tensor."""
    if ref.device.type == "cpu":
        ref = ref.float().to(dtype or got.dtype).to(DEV)
    return got.shape == ref.shape and torch.equal(got, ref)


class Kernels:
    """The C ABI of the BatchNorm family for one activation type."""

    def __init__(self, dtype):
        from structuredetector_amd import _lib as L
        self.L, self.lib, self.dtype, self.sfx = L, L.lib(), dtype, "_bf16" if dtype == BF16 else ""

    def call(self, name, *args, typed=True):
        self.L.check(getattr(self.lib, name + (self.sfx if typed else ""))(*args, self.L.stream()), name)

    def workspace(self, M, Cc):
        return nan_like_empty(self.lib.sd_col_reduce_workspace_bytes(M, Cc), torch.uint8)

    def train_sums(self, x, M, Cc):
        sums, ws = nan_like_empty(2 * Cc + 1, torch.float64), self.workspace(M, Cc)
        self.call("sd_bn_train_sums", ptr(x), M, Cc, ptr(sums), ptr(ws), ws.numel())
        return sums

    def train_stats(self, x, M, Cc, rm, rv):
        mean, invstd, ws = nan_like_empty(Cc, F32), nan_like_empty(Cc, F32), self.workspace(M, Cc)
        self.call("sd_bn_train_stats", ptr(x), M, Cc, R.EPS, R.MOMENTUM, ptr(rm), ptr(rv), ptr(mean), ptr(invstd), ptr(ws), ws.numel())
        return mean, invstd

    def stats_from_sums(self, sums, Cc, rm, rv):
        mean, invstd = nan_like_empty(Cc, F32), nan_like_empty(Cc, F32)
        self.call("sd_bn_stats_from_sums", ptr(sums), Cc, R.EPS, R.MOMENTUM, ptr(rm), ptr(rv), ptr(mean), ptr(invstd), typed=False)
        return mean, invstd

    def col_sum(self, x, M, Cc, out, accumulate):
        ws = self.workspace(M, Cc)
        self.call("sd_col_sum", ptr(x), M, Cc, ptr(out), accumulate, ptr(ws), ws.numel())

    def apply(self, x, M, Cc, P, res, relu, want_mask, offset=0):
        y = out_act(M, Cc, self.dtype, offset)
        mask = nan_like_empty(M * Cc // 4, torch.uint8) if want_mask else None
        self.call("sd_bn_apply", ptr(x), ptr(y), M, Cc, ptr(P.mean), ptr(P.invstd), ptr(P.gamma), ptr(P.beta), ptr(res), relu, ptr(mask))
        return y, mask

    def bwd_reduce(self, dy, x, y, relu, M, Cc, P, dgamma, dbeta, accumulate):
        sums, ws = nan_like_empty(2 * Cc + 1, torch.float64), self.workspace(M, Cc)
        self.call("sd_bn_bwd_reduce", ptr(dy), ptr(x), ptr(y), relu, M, Cc, ptr(P.mean), ptr(P.invstd), ptr(P.gamma), ptr(P.beta), ptr(dgamma),
                  ptr(dbeta), accumulate, ptr(sums), ptr(ws), ws.numel())
        return sums

    def means_from_sums(self, sums, Cc):
        means = nan_like_empty(2 * Cc, F32)
        self.call("sd_bn_bwd_means_from_sums", ptr(sums), Cc, ptr(means), typed=False)
        return means

    def bwd_apply(self, dy, x, y, relu, M, Cc, P, means, offset=0):
        dx, g_out = out_act(M, Cc, self.dtype, offset), out_act(M, Cc, self.dtype, offset)
        self.call("sd_bn_bwd_apply", ptr(dy), ptr(x), ptr(y), relu, M, Cc, ptr(P.mean), ptr(P.invstd), ptr(P.gamma), ptr(P.beta), ptr(means),
                  ptr(dx), ptr(g_out))
        return dx, g_out

    def bwd(self, dy, x, y, relu, M, Cc, P, dgamma, dbeta, accumulate, offset=0):
        dx, g_out, ws = out_act(M, Cc, self.dtype, offset), out_act(M, Cc, self.dtype, offset), self.workspace(M, Cc)
        self.call("sd_bn_bwd", ptr(dy), ptr(x), ptr(y), relu, M, Cc, ptr(P.mean), ptr(P.invstd), ptr(P.gamma), ptr(P.beta), ptr(dx), ptr(g_out),
                  ptr(dgamma), ptr(dbeta), accumulate, ptr(ws), ws.numel())
        return dx, g_out


def f32_add(prior, total):
    """prior + (float)total as the finish kernels accumulate: one fp32 addition."""
    return torch.from_numpy(prior.numpy().astype(np.float32) + total.numpy().astype(np.float32))


def run_case(case, d, M, Cc, dtype, exact, offset=0, relus=(0, 1, 2, 3)):
    """Forward statistics, sd_col_sum, the apply pass in three forms and the backward in the `relus` modes over one set of inputs."""
    k = Kernels(dtype)
    bf = dtype == BF16
    round_out = (lambda t: t.float().bfloat16().double()) if bf else (lambda t: t.float().double())
    store = (lambda ref: BF16_STORE * ref.abs()) if bf else (lambda ref: 0.0)
    p4 = R.plan(M, Cc)
    P = SimpleNamespace(mean=dev(d.mean), invstd=dev(d.invstd), gamma=dev(d.gamma), beta=dev(d.beta))
    x, dy, res = act(d.x, dtype, offset), act(d.dy, dtype, offset), act(d.res, dtype, offset)
    prior0, prior1 = d.prior0.float(), d.prior1.float().abs() + 0.5

    # ---- forward statistics: sums, the one-launch finish, the split finish ----
    S0, S1, A0 = R.stats_sums(d.x)
    sums_d = k.train_sums(x, M, Cc)
    sums = sums_d.cpu()
    assert sums[2 * Cc].item() == M
    if exact:
        assert torch.equal(sums[:Cc], S0) and torch.equal(sums[Cc:2 * Cc], S1), f"{case}: sum x / sum x^2 differ from the integer sums"
    else:
        b0, b1 = R.sum_bound(p4.L, A0), R.sum_bound(p4.L, S1)
        check_bound(case, "sum_x", sums[:Cc], S0, b0)
        check_bound(case, "sum_x2", sums[Cc:2 * Cc], S1, b1)
    rm, rv, rm2, rv2 = dev(prior0.clone()), dev(prior1.clone()), dev(prior0.clone()), dev(prior1.clone())
    mean, invstd = k.train_stats(x, M, Cc, rm, rv)
    mean2, invstd2 = k.stats_from_sums(sums_d, Cc, rm2, rv2)
    assert same(mean2, mean) and same(invstd2, invstd) and same(rm2, rm) and same(rv2, rv), f"{case}: split finish differs from the one-launch finish"
    t_mean, t_invstd, t_rm, t_rv = R.stats_tail(sums[:Cc], sums[Cc:2 * Cc], M, R.EPS, R.MOMENTUM, prior0, prior1)
    tiny = 2.0 ** -50
    check_tail(case, "mean", mean, t_mean)
    check_tail(case, "invstd", invstd, t_invstd)
    check_tail(case, "running_mean", rm, t_rm, tiny * (prior0.abs().double() + t_mean.abs()))
    check_tail(case, "running_var", rv, t_rv, tiny * prior1.double())
    if not exact:       # and against the truth, with the sum bounds carried through 1 / sqrt(S1/M - (S0/M)^2 + eps)
        _, inv_true, _, _ = R.stats_tail(S0, S1, M, R.EPS)
        bi = R.invstd_bound(S0, S1, b0, b1, M, R.EPS) + 2 * U * inv_true
        report(case, "invstd_bound_rel", (bi / inv_true).max().item())
        check_bound(case, "invstd_vs_fp64", invstd, inv_true, bi)

    # ---- column sums (bias gradient): overwrite, then accumulate onto prior contents ----
    D0, DA = d.dy.double().sum(0), d.dy.double().abs().sum(0)
    out0, out1 = nan_like_empty(Cc, F32), dev(prior0.clone())
    k.col_sum(dy, M, Cc, out0, 0)
    k.col_sum(dy, M, Cc, out1, 1)
    if exact:
        assert D0.abs().max().item() < 2 ** 24 and same(out0, D0) and same(out1, f32_add(prior0, D0)), f"{case}: sd_col_sum"
    else:
        check_bound(case, "col_sum", out0, D0, R.sum_bound(p4.L, DA))
        assert same(out1, f32_add(prior0, out0.cpu())), f"{case}: sd_col_sum accumulate"

    # ---- apply: plain, + ReLU + mask bytes, + residual + ReLU + mask bytes ----
    for relu, r_host, r_dev, want_mask in ((0, None, None, False), (1, None, None, True), (1, d.res, res, True)):
        what = f"apply_relu{relu}{'_res' if r_host is not None else ''}"
        pre, mag = R.pre_activation(d.x, d.mean, d.invstd, d.gamma, d.beta, r_host)
        yref = pre.clamp_min(0.0) if relu else pre
        y, mask = k.apply(x, M, Cc, P, r_dev, relu, want_mask, offset)
        if exact:
            assert same(y, yref), f"{case} {what}: y differs from the exact result"
        else:
            check_bound(case, what, y, yref, 6 * U * mag + store(yref))
        if want_mask:
            bits = R.unpack_mask(mask.cpu(), M, Cc)
            assert torch.equal(bits, y.cpu() > 0), f"{case} {what}: mask bits differ from y > 0"
            unsure = pre.abs() <= 6 * U * mag if not exact else torch.zeros_like(bits)
            assert unsure.double().mean().item() <= R.SKIP_CAP
            assert torch.equal(bits | unsure, (pre > 0) | unsure), f"{case} {what}: mask bits differ from pre-activation > 0"
            if exact:
                assert (pre == 0).any() and not bits[pre == 0].any(), f"{case} {what}: a zero pre-activation must give mask bit 0"
            if r_host is None:
                mask_plain = mask            # what the backward's relu = 2 recomputes

    # ---- backward in the four ReLU modes ----
    pre0, mag0 = R.pre_activation(d.x, d.mean, d.invstd, d.gamma, d.beta)
    if exact:
        y1_host = d.y1
        maskbytes = d.maskbytes
        unsure2 = torch.zeros(M, Cc, dtype=torch.bool)
    else:       # the saved post-activation and mask bytes of a residual layer
        prer, _ = R.pre_activation(d.x, d.mean, d.invstd, d.gamma, d.beta, d.res)
        y1_host = prer.clamp_min(0.0).float()
        y1_host = y1_host.bfloat16().float() if bf else y1_host
        maskbytes = R.pack_mask(prer > 0)
        unsure2 = pre0.abs() <= 6 * U * mag0
        assert unsure2.double().mean().item() <= R.SKIP_CAP
    y1 = act(y1_host, dtype, offset)
    mb = keep(torch.cat([maskbytes, torch.full((GUARD_ROWS * Cc // 4,), 0x0F, dtype=torch.uint8)]).to(DEV))[:M * Cc // 4]
    g_of_mode = {}
    for relu in relus:
        what = f"bwd_relu{relu}"
        wide = bf and Cc % 8 == 0 and relu != 1 and offset % 8 == 0
        L = R.plan(M, Cc, 8 if wide else 4).L
        yarg = {0: None, 1: y1, 2: None, 3: mb}[relu]
        keepmask = {0: None, 1: y1_host > 0, 2: pre0 > 0, 3: R.unpack_mask(maskbytes, M, Cc)}[relu]
        g = d.dy.double() if keepmask is None else d.dy.double() * keepmask
        skip = unsure2 if relu == 2 and not exact else None
        xhat, T0, T1, A0, A1 = R.bwd_terms(g, d.x, d.mean, d.invstd)
        # reduce half: fp64 sums, dgamma / dbeta overwritten, then accumulated onto prior contents
        dg0, db0, dg1, db1 = nan_like_empty(Cc, F32), nan_like_empty(Cc, F32), dev(prior0.clone()), dev(prior1.clone())
        sums_d = k.bwd_reduce(dy, x, yarg, relu, M, Cc, P, dg0, db0, 0)
        k.bwd_reduce(dy, x, yarg, relu, M, Cc, P, dg1, db1, 1)
        sums = sums_d.cpu()
        assert sums[2 * Cc].item() == M
        if exact:
            assert max(T0.abs().max().item(), T1.abs().max().item()) < 2 ** 24
            assert torch.equal(sums[:Cc], T0) and torch.equal(sums[Cc:2 * Cc], T1), f"{case} {what}: sum g / sum g*xhat differ from the exact sums"
            assert same(db0, T0) and same(dg0, T1) and same(db1, f32_add(prior1, T0)) and same(dg1, f32_add(prior0, T1)), f"{case} {what}: dgamma / dbeta"
        else:
            s0 = s1 = 0.0
            if skip is not None:        # an undecidable ReLU may add or drop its whole term
                s0, s1 = (d.dy.double().abs() * skip).sum(0), ((d.dy.double() * xhat).abs() * skip).sum(0)
            check_bound(case, what + "_sum_g", sums[:Cc], T0, R.sum_bound(L, A0) + s0)
            check_bound(case, what + "_sum_gxhat", sums[Cc:2 * Cc], T1, R.sum_bound(L, A1) + s1)
            check_tail(case, what + "_dbeta", db0, sums[:Cc])
            check_tail(case, what + "_dgamma", dg0, sums[Cc:2 * Cc])
            assert same(db1, f32_add(prior1, db0.cpu())) and same(dg1, f32_add(prior0, dg0.cpu())), f"{case} {what}: accumulate"
        means_d = k.means_from_sums(sums_d, Cc)
        means = means_d.cpu()
        check_tail(case, what + "_mean_g", means[:Cc], sums[:Cc] / M)
        check_tail(case, what + "_mean_gxhat", means[Cc:], sums[Cc:2 * Cc] / M)
        # apply half with the library's own means ...
        dx, g_out = k.bwd_apply(dy, x, yarg, relu, M, Cc, P, means_d, offset)
        dref, dmag = R.bwd_apply(g, xhat, d.gamma, d.invstd, means[:Cc], means[Cc:])
        check_bound(case, what + "_dx", dx, dref, 8 * U * dmag + store(dref), skip)
        g_host = g_out.cpu().double()
        assert torch.equal(g_host if skip is None else g_host.masked_fill(skip, 0.0), g if skip is None else g.masked_fill(skip, 0.0)), \
            f"{case} {what}: g_out is not dy or 0"
        g_of_mode[relu] = g_out
        if exact:       # ... with dyadic means every product is exact; a zero pre-activation / post-activation passes no gradient
            dx_e, _ = k.bwd_apply(dy, x, yarg, relu, M, Cc, P, dev(torch.cat([d.mg, d.mgx])), offset)
            eref, _ = R.bwd_apply(g, xhat, d.gamma, d.invstd, d.mg, d.mgx)
            assert same(dx_e, round_out(eref)), f"{case} {what}: dx differs from the exact result"
            zero = {1: y1_host == 0, 2: pre0 == 0}.get(relu)
            if zero is not None:
                assert (zero & (d.dy != 0)).any() and not g_host[zero].any(), f"{case} {what}: gradient through a zero activation"
        # the one call equals reduce -> means -> apply, bit for bit
        dgf, dbf = nan_like_empty(Cc, F32), nan_like_empty(Cc, F32)
        dx_f, g_f = k.bwd(dy, x, yarg, relu, M, Cc, P, dgf, dbf, 0, offset)
        assert same(dx_f, dx) and same(g_f, g_out) and same(dgf, dg0) and same(dbf, db0), f"{case} {what}: sd_bn_bwd differs from its split form"
    if 2 in g_of_mode:   # the mask recomputed from x is the mask the forward wrote: no skipped elements here
        _, g3 = k.bwd_apply(dy, x, mask_plain, 3, M, Cc, P, dev(torch.zeros(2 * Cc)), offset)
        assert same(g3, g_of_mode[2]), f"{case}: relu = 2 recomputes another mask than sd_bn_apply wrote"


BF16_STORE = R.BF16_U
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]


def test_launch_shape_restatement_matches_the_library():
    """bn_ref.plan / fold_rows restate red_rows / fold_rows of the host code: the sum bounds are built on them."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    for M, Cc in list(R.SHAPES.values()) + [(1, 4), (16384, 512), (262144, 64), (1048576, 64), (2 ** 21 + 3, 1024)]:
        assert lib.sd_col_reduce_workspace_bytes(M, Cc) == R.plan(M, Cc).workspace_bytes, (M, Cc)
    for rows in [r for r, _ in R.ROW_CASES.values()] + [2047, 2050, 2110, 4096, 8191, 100000]:
        assert lib.sd_bn_finalize_scratch_rows(rows) == R.fold_rows(rows), rows


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_whole_tensor_exact(name, dtype):
    """Integer inputs: every sum equals the int64 sum, every elementwise result the exact one, in fp32 and bf16."""
    M, Cc = R.SHAPES[name]
    run_case(f"{name}-exact-{'bf16' if dtype == BF16 else 'f32'}", R.exact_inputs(M, Cc), M, Cc, dtype, exact=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_whole_tensor_random(name, dtype):
    """Gaussian inputs with per-channel scale and offset against the fp64 reference, inside the derived bounds."""
    M, Cc = R.SHAPES[name]
    bf = dtype == BF16
    run_case(f"{name}-random-{'bf16' if bf else 'f32'}", R.random_inputs(M, Cc, seed=1, bf16=bf), M, Cc, dtype, exact=False)


@pytest.mark.parametrize("name", ["rpb64_ragged_f32_grid_stride", "c4_256_lanes_tail_block"])
def test_whole_tensor_mean_32_sigma(name):
    """|mu| / sigma = 32 in every channel: the variance S1/M - mean^2 cancels five digits of its fp32 block partials.  Same derived bounds
    (they allow invstd 0.2 % - 3 % here); the forward statistics, the apply pass and the mask-recomputing backward, fp32."""
    M, Cc = R.SHAPES[name]
    run_case(f"{name}-mean32sigma-f32", R.random_inputs(M, Cc, seed=2, ratio=32.0), M, Cc, F32, exact=False, relus=(2,))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("offset,Cc", [(0, 64), (4, 64), (0, 4), (0, 8)], ids=["wide_aligned16_c64", "narrow_offset8_c64", "narrow_c4", "wide_c8"])
def test_bf16_kernel_choice(offset, Cc, exact):
    """sd_bn_apply_bf16 / sd_bn_bwd_bf16 / sd_bn_bwd_reduce_bf16 / sd_bn_bwd_apply_bf16 pick the 16-byte kernels for C % 8 == 0, relu != 1
    and 16-byte aligned activations, the 8-byte templated ones otherwise: 16-byte aligned buffers, every activation pointer advanced by 8
    bytes, C = 4; relu = 1 is narrow by rule in every variant.  In the exact regime all of them equal the exact result, hence each other."""
    M = 421
    d = R.exact_inputs(M, Cc, seed=4) if exact else R.random_inputs(M, Cc, seed=4, bf16=True)
    x = act(d.x, BF16, offset)
    assert x.data_ptr() % 16 == (8 if offset else 0)
    run_case(f"bf16_choice-off{offset}-c{Cc}-{'exact' if exact else 'random'}", d, M, Cc, BF16, exact, offset=offset)


def _partial_rows(rows, Cc, exact, seed):
    g = torch.Generator().manual_seed(seed)
    if exact:
        return torch.randint(-500, 501, (rows, 2 * Cc), generator=g).float()
    c = torch.arange(2 * Cc)
    return (torch.randn(rows, 2 * Cc, generator=g).double() * 2.0 ** ((c % 8) - 2).double() + ((c % 3) - 1).double() * 3).float()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("name", list(R.ROW_CASES))
def test_finish_kernels_on_synthetic_partial_rows(name, exact):
    """sd_bn_stats_sums / sd_bn_finalize_stats / sd_bn_bwd_sums / sd_bn_bwd_finalize on caller-made partial rows [rows][2][C], with and
    without the fold scratch: k_rows_fold (slabs, idle lanes, ragged last slab), the 512-row trips of col_pair_sums and their ragged last
    trip.  Sums against the fp64 column sums (equal in the exact regime, (L_fold + 2) u sum|p| otherwise, the same bound with scratch = NULL);
    the outputs against the formulas on the sums the library returned."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    rows, Cc = R.ROW_CASES[name]
    case = f"rows-{name}-{'exact' if exact else 'random'}"
    M = rows * 16 + 5
    part = _partial_rows(rows, Cc, exact, seed=rows)
    assert exact is False or (part[0] != 0).any()                  # col_pair_sums re-reads row 0 for the rows a trip does not have
    buf = keep(torch.full(((rows + 64) * 2 * Cc,), 3.0, device=DEV))       # 64 guard rows: one slab of k_rows_fold at the most
    pd = buf[:rows * 2 * Cc].view(rows, 2 * Cc)
    pd.copy_(part.to(DEV))
    ref, ref_abs = part.double().sum(0), part.double().abs().sum(0)
    fold = R.fold_plan(rows, Cc)
    bound = R.sum_bound(fold.L if fold else 0, ref_abs)
    prior0, prior1 = R.exact_params(Cc).prior0, R.exact_params(Cc).prior1.abs() + 0.5
    results = []
    for with_scratch in (True, False):
        tag = "scratch" if with_scratch else "noscratch"
        scratch = nan_like_empty(max(lib.sd_bn_finalize_scratch_rows(rows), 1) * 2 * Cc, F32) if with_scratch else None
        st = L.stream()
        # forward: sums, then the one-launch finish against the formula on them
        fs = nan_like_empty(2 * Cc + 1, torch.float64)
        L.check(lib.sd_bn_stats_sums(ptr(pd), rows, M, Cc, ptr(fs), ptr(scratch), st))
        mean, invstd, rm, rv = nan_like_empty(Cc, F32), nan_like_empty(Cc, F32), dev(prior0.clone()), dev(prior1.clone())
        L.check(lib.sd_bn_finalize_stats(ptr(pd), rows, M, Cc, R.EPS, R.MOMENTUM, ptr(rm), ptr(rv), ptr(mean), ptr(invstd), ptr(scratch), st))
        # backward: sums + dgamma / dbeta (overwrite, accumulate), then the one-launch finish
        bs, dg0, db0, dg1, db1 = nan_like_empty(2 * Cc + 1, torch.float64), nan_like_empty(Cc, F32), nan_like_empty(Cc, F32), dev(prior0.clone()), dev(prior1.clone())
        L.check(lib.sd_bn_bwd_sums(ptr(pd), rows, M, Cc, ptr(dg0), ptr(db0), 0, ptr(bs), ptr(scratch), st))
        L.check(lib.sd_bn_bwd_sums(ptr(pd), rows, M, Cc, ptr(dg1), ptr(db1), 1, ptr(bs), ptr(scratch), st))
        means, dgf, dbf, dgf1, dbf1 = nan_like_empty(2 * Cc, F32), nan_like_empty(Cc, F32), nan_like_empty(Cc, F32), dev(prior0.clone()), dev(prior1.clone())
        L.check(lib.sd_bn_bwd_finalize(ptr(pd), rows, M, Cc, ptr(dgf), ptr(dbf), 0, ptr(means), ptr(scratch), st))
        L.check(lib.sd_bn_bwd_finalize(ptr(pd), rows, M, Cc, ptr(dgf1), ptr(dbf1), 1, ptr(means), ptr(scratch), st))
        fsh, bsh = fs.cpu(), bs.cpu()
        assert fsh[2 * Cc].item() == M and bsh[2 * Cc].item() == M
        assert torch.equal(fsh, bsh), f"{case} {tag}: forward and backward finish sum the same rows differently"
        if exact:
            assert ref.abs().max().item() < 2 ** 24 and torch.equal(fsh[:2 * Cc], ref), f"{case} {tag}: sums differ from the integer sums"
        else:
            check_bound(case, f"sums_{tag}", fsh[:2 * Cc], ref, bound)
        t_mean, t_invstd, t_rm, t_rv = R.stats_tail(fsh[:Cc], fsh[Cc:2 * Cc], M, R.EPS, R.MOMENTUM, prior0, prior1)
        check_tail(case, f"mean_{tag}", mean, t_mean)
        check_tail(case, f"invstd_{tag}", invstd, t_invstd)
        check_tail(case, f"running_mean_{tag}", rm, t_rm, 2.0 ** -50 * (prior0.abs().double() + t_mean.abs()))
        check_tail(case, f"running_var_{tag}", rv, t_rv, 2.0 ** -50 * prior1.double())
        check_tail(case, f"dbeta_{tag}", db0, bsh[:Cc])
        check_tail(case, f"dgamma_{tag}", dg0, bsh[Cc:2 * Cc])
        check_tail(case, f"means_{tag}", means, bsh[:2 * Cc] / M)
        assert same(dgf, dg0) and same(dbf, db0) and same(dgf1, dg1) and same(dbf1, db1), f"{case} {tag}: one-launch finish differs from the split one"
        assert same(db1, f32_add(prior1, db0.cpu())) and same(dg1, f32_add(prior0, dg0.cpu())), f"{case} {tag}: accumulate"
        if exact:
            assert same(db0, ref[:Cc]) and same(dg0, ref[Cc:])
        results.append((fsh, mean, invstd, means))
    if exact:
        (a, m0, i0, n0), (b, m1, i1, n1) = results
        assert torch.equal(a, b) and same(m1, m0) and same(i1, i0) and same(n1, n0), f"{case}: the fold changes an exact sum"


@pytest.mark.parametrize("Cc", [1, 4, 255, 257, 1024])
def test_bn_fold(Cc):
    """Eval-mode fold scale = gamma / sqrt(rv + eps), shift = beta - rm * scale at channel counts around the 256-thread block (no C % 4
    rule here): 4u relative on scale, 4u (|beta| + |rm * scale|) on shift; nothing is written past channel C - 1."""
    from structuredetector_amd import _lib as L
    g = torch.Generator().manual_seed(Cc)
    gamma, beta, rm, rv = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 3, torch.rand(Cc, generator=g) * 4 + 0.01
    scale, shift = nan_like_empty(Cc + 8, F32), nan_like_empty(Cc + 8, F32)
    L.check(L.lib().sd_bn_fold(ptr(dev(gamma)), ptr(dev(beta)), ptr(dev(rm)), ptr(dev(rv)), R.EPS, Cc, ptr(scale), ptr(shift), L.stream()))
    s_ref, h_ref = R.bn_fold(gamma, beta, rm, rv)
    check_bound(f"fold-c{Cc}", "scale", scale[:Cc], s_ref, 4 * U * s_ref.abs())
    check_bound(f"fold-c{Cc}", "shift", shift[:Cc], h_ref, 4 * U * (beta.double().abs() + (rm.double() * s_ref).abs()))
    assert torch.isnan(scale[Cc:]).all() and torch.isnan(shift[Cc:]).all()


def test_statistics_tail_edge_cases():
    """One row (the unbiased variance falls back to the biased one: 0), a constant channel (var = 0, invstd = 1 / sqrt(eps)) and the momentum
    update from non-trivial running statistics, against the fp64 formula on the library's own sums."""
    k = Kernels(F32)
    g = torch.Generator().manual_seed(8)
    for M, Cc in ((1, 64), (50, 8)):
        x = torch.randint(-3, 4, (M, Cc), generator=g).float() if M == 1 else torch.randn(M, Cc, generator=g)
        if M > 1:
            x[:, 3] = 3.0
            x[:, 5] = 0.0
        prior0, prior1 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
        xd, rm, rv = act(x, F32), dev(prior0.clone()), dev(prior1.clone())
        sums = k.train_sums(xd, M, Cc).cpu()
        mean, invstd = k.train_stats(xd, M, Cc, rm, rv)
        t_mean, t_invstd, t_rm, t_rv = R.stats_tail(sums[:Cc], sums[Cc:2 * Cc], M, R.EPS, R.MOMENTUM, prior0, prior1)
        case = f"tail-M{M}"
        check_tail(case, "mean", mean, t_mean)
        check_tail(case, "invstd", invstd, t_invstd)
        check_tail(case, "running_mean", rm, t_rm, 2.0 ** -50 * (prior0.abs().double() + t_mean.abs()))
        check_tail(case, "running_var", rv, t_rv, 2.0 ** -50 * prior1.double())
        const = torch.arange(Cc) if M == 1 else torch.tensor([3, 5])
        top = torch.full((len(const),), float(np.float32(R.EPS)) ** -0.5, dtype=torch.float64)
        check_tail(case, "invstd_constant_channel", invstd.cpu()[const], top)
        check_tail(case, "running_var_constant_channel", rv.cpu()[const], (1.0 - R.MOMENTUM) * prior1[const].double())
        assert torch.equal(mean.cpu()[const].double(), x[0, const].double())
