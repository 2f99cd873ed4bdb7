"""The optimizer choice on the GPU: `sd_sgd_step` against torch.optim.SGD (one param group per id, clip_grad_norm_, the EMA recurrence
written out) and `sd_lamb_step` against the LAMB formulas written out below with torch tensor ops per slot; `TrainStep(optimizer=...)` on
the small net, resume, and the command line.  Conventions of tests/test_gpu_optim.py: hyper-parameters pre-rounded to fp32, truth in
fp64, the same reference in fp32 printed beside every figure (`pytest -s`).

Bound in force, every buffer (parameters, state buffers, EMA) of every case: ADAM_TOL = 1e-6 of the buffer's largest value -- no LAMB
case needed the wider bound the trust ratio would have allowed (the data keeps phi of order 1: about 0.5).  Status norm: 1e-6 relative.  Expected
values never come from the code under test."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_optim import ADAM_TOL, B1, B2, EPS, _small_step_setup, _Spy, f32, new_status, read_status, sumsq

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCK, MAX_SLOT_BLOCKS = 4096, 128                  # SD_LAMB_BLOCK_FLOATS, SD_LAMB_MAX_SLOT_BLOCKS
LR_SGD, LR_LAMB, WD, GSCALE = f32(1e-2), f32(2e-3), f32(0.05), 0.5
LR_MUL, WD_MUL = [1.0, 0.0, 0.5], [1.0, 1.0, 0.0]   # three groups: distinct rates (one of them 0) and decays


def floats(values):
    return (C.c_float * len(values))(*values)


def f32mul(a, b):
    """One fp32 multiply of two fp32 arguments, as the entry points form lr_k and wd_k."""
    return float(np.float32(a) * np.float32(b))


# ---- calling the entry points -------------------------------------------------------------------------------------------------------------
def build_table(lib, slots, n):
    """sd_lamb_table_build on the host, the table uploaded -> (device table, nslots, nblocks)."""
    from structuredetector_amd import _lib as L
    count = len(slots)
    lo, hi = (C.c_int64 * count)(*(s[0] for s in slots)), (C.c_int64 * count)(*(s[1] for s in slots))
    adapt = (C.c_ubyte * count)(*(int(s[2]) for s in slots))
    need, blocks = C.c_size_t(), C.c_int()
    L.check(lib.sd_lamb_table_build(lo, hi, adapt, count, n, None, 0, C.byref(need), C.byref(blocks)), "sd_lamb_table_build")
    host = torch.zeros(need.value // 4, dtype=torch.int32)
    L.check(lib.sd_lamb_table_build(lo, hi, adapt, count, n, host.data_ptr(), need.value, None, None), "sd_lamb_table_build")
    return host.to(DEV), count, blocks.value


def sgd_step(lib, p, g, buf, ids, lr_mul, wd_mul, lr=LR_SGD, momentum=0.0, nesterov=False, gscale=1.0, wd=0.0, max_norm=0.0, ema=None,
             ema_decay=0.0, status=None, partials=None, n=None):
    from structuredetector_amd import _lib as L
    n = p.numel() if n is None else n
    if max_norm > 0:
        partials = sumsq(lib, g[:n], partials)
    L.check(lib.sd_sgd_step(p.data_ptr(), g.data_ptr(), None if buf is None else buf.data_ptr(), n, lr, momentum, int(nesterov), gscale, wd,
                            ids.data_ptr(), floats(lr_mul), floats(wd_mul), len(lr_mul), max_norm, None if partials is None else partials.data_ptr(),
                            0 if partials is None else partials.numel(), None if ema is None else ema.data_ptr(), ema_decay,
                            None if status is None else status.data_ptr(), L.stream()), "sd_sgd_step")
    torch.cuda.synchronize()


def lamb_step(lib, p, g, m, v, step, ids, lr_mul, wd_mul, table, lr=LR_LAMB, gscale=1.0, wd=0.0, max_norm=0.0, ema=None, ema_decay=0.0,
              status=None, partials=None, ws=None, n=None):
    from structuredetector_amd import _lib as L
    n = p.numel() if n is None else n
    tab, nslots, nblocks = table
    if ws is None:
        ws = torch.empty(lib.sd_lamb_workspace_bytes(nblocks) // 8, dtype=torch.float64, device=DEV)
    if max_norm > 0:
        partials = sumsq(lib, g[:n], partials)
    L.check(lib.sd_lamb_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, lr, B1, B2, EPS, gscale, wd, ids.data_ptr(),
                             floats(lr_mul), floats(wd_mul), len(lr_mul), max_norm, None if partials is None else partials.data_ptr(),
                             0 if partials is None else partials.numel(), None if ema is None else ema.data_ptr(), ema_decay,
                             None if status is None else status.data_ptr(), tab.data_ptr(), nslots, nblocks, ws.data_ptr(), ws.numel() * 8,
                             L.stream()), "sd_lamb_step")
    torch.cuda.synchronize()


# ---- references -----------------------------------------------------------------------------------------------------------------------------
class TorchSgd:
    """torch.optim.SGD itself (dampening 0) with one param group per id, clip_grad_norm_ over all groups before each step.  `step` takes
    the averaged gradient, optionally the parameters to start from (`TrainStep`: the step's own parameters before the step)."""

    def __init__(self, dtype, p0, elem_ids, lrs, wds, momentum, nesterov):
        self.dtype, self.numel = dtype, p0.numel()
        self.sel = [(elem_ids == k).nonzero().squeeze(1) for k in range(len(lrs))]
        self.params = [p0[s].to(dtype).clone().requires_grad_(True) for s in self.sel]
        self.opt = torch.optim.SGD([dict(params=[q], lr=lrs[k], weight_decay=wds[k]) for k, q in enumerate(self.params) if q.numel()], lr=1.0,
                                   momentum=momentum, dampening=0.0, nesterov=nesterov)

    def flat(self, parts):
        out = torch.zeros(self.numel, dtype=self.dtype)
        for s, part in zip(self.sel, parts):
            if part is not None:
                out[s] = part
        return out

    def step(self, grad, max_norm=0.0, start=None):
        for s, q in zip(self.sel, self.params):
            if start is not None:
                q.data.copy_(start[s].to(self.dtype))
            q.grad = grad[s].to(self.dtype).clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(self.params, max_norm)
        self.opt.step()
        return self.flat([q.detach() for q in self.params])

    def momentum_buffer(self):
        return self.flat([self.opt.state[q].get("momentum_buffer") if q in self.opt.state else None for q in self.params])


def lamb_reference_step(dtype, p, g, m, v, t, slots, lr_elem, wd_elem, max_norm):
    """One LAMB step, written out (You et al. 2020, Alg. 2, with the adapt bit per slot): g the averaged gradient, lr_elem / wd_elem the
    per-element lr_k / wd_k.  Returns the new (p, m, v)."""
    p, g, m, v = p.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype)
    lr_elem, wd_elem = lr_elem.to(dtype), wd_elem.to(dtype)
    if max_norm > 0:
        g = g * min(1.0, max_norm / (float(g.norm()) + 1e-6))
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    u = (m / (1 - B1 ** t)) / ((v / (1 - B2 ** t)).sqrt() + EPS) + wd_elem * p
    new = p.clone()
    for lo, hi, adapt in slots:
        norm_p, norm_u = float(p[lo:hi].norm()), float(u[lo:hi].norm())
        phi = norm_p / norm_u if adapt and norm_p > 0 and norm_u > 0 and math.isfinite(norm_p) and math.isfinite(norm_u) else 1.0
        new[lo:hi] = p[lo:hi] - lr_elem[lo:hi] * phi * u[lo:hi]
    return new, m, v


def close(name, got, want, yard=None, tol=ADAM_TOL):
    """|got - want| <= tol * max|want|, printed beside the fp32 reference's own error."""
    got, want = got.detach().cpu().double(), want.double()
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    err32 = float("nan") if yard is None else (yard.double() - want).abs().max().item()
    print(f"{name}: err {err:.3e}, err/scale {err / scale if scale else 0:.3e}, fp32 reference err/scale {err32 / scale if scale else 0:.3e}")
    assert err <= tol * scale, f"{name}: {err:.3e} vs fp64 (bound {tol * scale:.3e}), fp32 reference {err32:.3e}, scale {scale:.3e}"


# ---- the kernel-level layout: slots of 8, 8 with one padding float, one block, one block + 8, three blocks + 8, a ragged last one ----------
SIZES = [8, 8, BLOCK, BLOCK + 8, 3 * BLOCK + 8, 5000]
ADAPT = [True, True, False, True, True, False]
SLOT_GROUP = [0, 2, 1, 2, 0, 1]                     # the group of each slot (group 1 stands still: lr_mul 0)
PAD = 15                                            # the last float of slot 1: padding (p = 0, g = 0)


def _layout():
    lo = [sum(SIZES[:k]) for k in range(len(SIZES))]
    slots = [(a, a + s, ad) for a, s, ad in zip(lo, SIZES, ADAPT)]
    n = slots[-1][1]
    ids = torch.zeros(n // 4, dtype=torch.uint8)
    for (a, b, _), k in zip(slots, SLOT_GROUP):
        ids[a // 4:b // 4] = k
    return slots, n, ids


@pytest.fixture(scope="module")
def data():
    """Parameters, five averaged gradients and the EMA decays shared by the kernel-level cases (never modified)."""
    slots, n, ids = _layout()
    g = torch.Generator().manual_seed(2020)
    p0 = torch.randn(n, generator=g) * 0.5           # |p| / |u| is then about 0.5: a trust ratio that shows
    grads = [torch.randn(n, generator=g) * 0.02 for _ in range(5)]
    p0[PAD] = 0.0
    for gr in grads:
        gr[PAD] = 0.0
    norm0 = float(grads[0].double().norm())
    return dict(slots=slots, n=n, ids=ids, elem_ids=ids.repeat_interleave(4).long(), p0=p0, grads=grads,
                ema_decays=[f32(min(0.99, (1 + t) / (10 + t))) for t in range(1, 6)],
                max_norms=dict(off=0.0, below=f32(100 * norm0), above=f32(0.01 * norm0)))


def _ema_reference(dtype, p0, params, decays):
    ema = p0.to(dtype).clone()
    for p, d in zip(params, decays):
        ema = d * ema + (1 - d) * p.to(dtype)
    return ema


@pytest.mark.parametrize("clip", ["off", "below", "above"])
@pytest.mark.parametrize("momentum, nesterov", [(0.0, False), (f32(0.9), False), (f32(0.9), True)])
def test_sgd_five_steps_against_torch_sgd(data, momentum, nesterov, clip):
    from structuredetector_amd import _lib as L
    lib = L.lib()
    n, p0, max_norm = data["n"], data["p0"], data["max_norms"][clip]
    lrs, wds = [f32mul(LR_SGD, x) for x in LR_MUL], [f32mul(WD, x) for x in WD_MUL]
    refs = {}
    for dtype in (torch.float64, torch.float32):
        ref = TorchSgd(dtype, p0, data["elem_ids"], lrs, wds, momentum, nesterov)
        steps = [ref.step(gr, max_norm) for gr in data["grads"]]
        refs[dtype] = (steps[-1], ref.momentum_buffer(), _ema_reference(dtype, p0, steps, data["ema_decays"]))
    p, ema, status = p0.to(DEV), p0.to(DEV), new_status()
    buf = torch.zeros(n, device=DEV) if momentum else None
    for gr, d in zip(data["grads"], data["ema_decays"]):
        sgd_step(lib, p, (gr / GSCALE).to(DEV), buf, data["ids"].to(DEV), LR_MUL, WD_MUL, momentum=momentum, nesterov=nesterov, gscale=GSCALE, wd=WD,
                 max_norm=max_norm, ema=ema, ema_decay=d, status=status)
    want, yard = refs[torch.float64], refs[torch.float32]
    close("param", p, want[0], yard[0])
    close("ema", ema, want[2], yard[2])
    if momentum:
        close("momentum_buf", buf, want[1], yard[1])
    if max_norm:
        norm, coef, skipped = read_status(status)
        true_norm = float(data["grads"][-1].double().norm())
        print(f"status norm {norm:.9e}, fp64 {true_norm:.9e}")
        assert abs(norm - true_norm) <= 1e-6 * true_norm and skipped == 0
        assert coef == 1.0 if clip == "below" else 0 < coef < 0.011
    still = data["elem_ids"] == 1                   # lr_mul = 0: the parameter stands, its momentum still builds up
    assert torch.equal(p.cpu()[still], p0[still]) and (not momentum or float(buf.cpu()[still].abs().max()) > 0)
    assert float(p[PAD]) == 0.0 and float(ema[PAD]) == 0.0 and (buf is None or float(buf[PAD]) == 0.0)
    assert not torch.equal(p.cpu()[~still], p0[~still])


def _lamb_run(lib, data, max_norm, dtype=None, ws_fill=None):
    """Five steps: the kernels (dtype None; returns device buffers and the status) or the written-out reference in `dtype`."""
    n, p0, slots = data["n"], data["p0"], data["slots"]
    lr_elem = torch.tensor([f32mul(LR_LAMB, x) for x in LR_MUL], dtype=torch.float64)[data["elem_ids"]]
    wd_elem = torch.tensor([f32mul(WD, x) for x in WD_MUL], dtype=torch.float64)[data["elem_ids"]]
    if dtype is not None:
        p, m, v, ema = p0.to(dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype), p0.to(dtype)
        for t, (gr, d) in enumerate(zip(data["grads"], data["ema_decays"]), 1):
            p, m, v = lamb_reference_step(dtype, p, gr, m, v, t, slots, lr_elem, wd_elem, max_norm)
            ema = d * ema + (1 - d) * p
        return p, m, v, ema
    table = build_table(lib, slots, n)
    p, m, v, ema, status = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(DEV), new_status()
    ws = None if ws_fill is None else torch.full((2 * table[2],), ws_fill, dtype=torch.float64, device=DEV)
    for t, (gr, d) in enumerate(zip(data["grads"], data["ema_decays"]), 1):
        lamb_step(lib, p, (gr / GSCALE).to(DEV), m, v, t, data["ids"].to(DEV), LR_MUL, WD_MUL, table, gscale=GSCALE, wd=WD, max_norm=max_norm, ema=ema,
                  ema_decay=d, status=status, ws=ws)
    return p, m, v, ema, status


@pytest.mark.parametrize("clip", ["off", "below", "above"])
def test_lamb_five_steps_against_the_written_out_formulas(data, clip):
    from structuredetector_amd import _lib as L
    max_norm = data["max_norms"][clip]
    want, yard = _lamb_run(None, data, max_norm, torch.float64), _lamb_run(None, data, max_norm, torch.float32)
    got = _lamb_run(L.lib(), data, max_norm)
    for name, a, w, y in zip(("param", "exp_avg", "exp_avg_sq", "ema"), got, want, yard):
        close(name, a, w, y)
    p, p0, elem_ids = got[0].cpu(), data["p0"], data["elem_ids"]
    if max_norm:
        norm, coef, skipped = read_status(got[4])
        true_norm = float(data["grads"][-1].double().norm())
        print(f"status norm {norm:.9e}, fp64 {true_norm:.9e}")
        assert abs(norm - true_norm) <= 1e-6 * true_norm and skipped == 0
        assert coef == 1.0 if clip == "below" else 0 < coef < 0.011
    still = elem_ids == 1
    assert torch.equal(p[still], p0[still]) and float(got[1].cpu()[still].abs().max()) > 0 and float(got[2].cpu()[still].abs().max()) > 0
    for buf in got[:4]:
        assert float(buf[PAD]) == 0.0, "a padding float (p = 0, g = 0) stays exactly 0"
    # the trust ratio is really applied: an adapted slot moved by another amount than the plain formula gives
    lo, hi, _ = data["slots"][4]
    plain = [(a, b, False) for a, b, _ in data["slots"]]
    lr_elem = torch.tensor([f32mul(LR_LAMB, x) for x in LR_MUL], dtype=torch.float64)[elem_ids]
    wd_elem = torch.tensor([f32mul(WD, x) for x in WD_MUL], dtype=torch.float64)[elem_ids]
    q, m, v = p0.double(), torch.zeros(p0.numel(), dtype=torch.float64), torch.zeros(p0.numel(), dtype=torch.float64)
    for t, gr in enumerate(data["grads"], 1):
        q, m, v = lamb_reference_step(torch.float64, q, gr, m, v, t, plain, lr_elem, wd_elem, max_norm)
    assert (q[lo:hi] - want[0][lo:hi]).abs().max().item() > 100 * ADAM_TOL * want[0].abs().max().item()
    # ... and a non-adapted slot equals the plain formula
    lo, hi, adapt = data["slots"][5]
    assert not adapt
    close("non-adapted slot", got[0][lo:hi], q[lo:hi])


def test_lamb_edge_slots():
    """p all zero (phi = 1: the slot moves by lr * u); gradient and moments all zero without decay (u = 0: phi = 1, no NaN, unchanged);
    a non-adapted slot (the plain formula); padding floats stay exactly 0."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    slots = [(0, 16, True), (16, 32, True), (32, 40, False), (40, 40 + BLOCK, True)]
    n = slots[-1][1]
    ids = torch.zeros(n // 4, dtype=torch.uint8)
    ids[4:8] = 1                                     # slot 1: the group without decay
    g = torch.Generator().manual_seed(3)
    p0, gr = torch.randn(n, generator=g) * 0.5, torch.randn(n, generator=g) * 0.02
    p0[0:16] = 0.0
    gr[16:32] = 0.0
    p0[39] = gr[39] = 0.0                            # the padding float of slot 2
    lr_mul, wd_mul = [1.0, 1.0], [1.0, 0.0]
    elem_ids = ids.repeat_interleave(4).long()
    lr_elem = torch.tensor([f32mul(LR_LAMB, x) for x in lr_mul], dtype=torch.float64)[elem_ids]
    wd_elem = torch.tensor([f32mul(WD, x) for x in wd_mul], dtype=torch.float64)[elem_ids]
    z = torch.zeros(n, dtype=torch.float64)
    want = lamb_reference_step(torch.float64, p0, gr, z, z, 1, slots, lr_elem, wd_elem, 0.0)
    yard = lamb_reference_step(torch.float32, p0, gr, z, z, 1, slots, lr_elem, wd_elem, 0.0)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    lamb_step(lib, p, gr.to(DEV), m, v, 1, ids.to(DEV), lr_mul, wd_mul, build_table(lib, slots, n), wd=WD)
    for name, a, w, y in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), want, yard):
        assert bool(torch.isfinite(a).all()), name
        close(name, a, w, y)
    p = p.cpu()
    # slot 0: p = 0, so u = m_hat / (sqrt(v_hat) + eps) = sign(g) at step 1, and the slot moves by lr * u with phi = 1
    step1 = (gr[0:16].double() / (gr[0:16].double().abs() + EPS)) * LR_LAMB
    assert (p[0:16].double() + step1).abs().max().item() <= 1e-6 * LR_LAMB
    assert torch.equal(p[16:32], p0[16:32])          # u = 0: unchanged, bit for bit
    assert float(p[39]) == 0.0 and float(m[39]) == 0.0 and float(v[39]) == 0.0
    u = (gr.double() / (gr.double().abs() + EPS)) + wd_elem * p0.double()
    assert (p[32:40].double() - (p0[32:40].double() - LR_LAMB * u[32:40])).abs().max().item() <= ADAM_TOL * p0[32:40].abs().max().item()
    lo, hi, _ = slots[3]                             # the adapted slot moved by phi * lr * u, phi = |p| / |u| written out
    phi = float(p0[lo:hi].double().norm() / u[lo:hi].norm())
    assert abs(phi - 1) > 0.01
    assert (p[lo:hi].double() - (p0[lo:hi].double() - LR_LAMB * phi * u[lo:hi])).abs().max().item() <= ADAM_TOL * p0[lo:hi].abs().max().item()


# ---- determinism, the guard, a wrong table ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """One slot larger than a sweep of its 128 blocks (128 blocks' worth + one block + 8 floats) behind a slot of 8."""
    slots = [(0, 8, False), (8, 8 + MAX_SLOT_BLOCKS * BLOCK + BLOCK + 8, True)]
    n = slots[-1][1]
    g = torch.Generator().manual_seed(11)
    return dict(slots=slots, n=n, ids=torch.zeros(n // 4, dtype=torch.uint8), p0=torch.randn(n, generator=g),
                grads=[torch.randn(n, generator=g) * 0.02 for _ in range(2)])


def _big_run(lib, big, kind, fill, poison=None):
    n = big["n"]
    p, m, v, ema, status = big["p0"].to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), big["p0"].to(DEV), new_status()
    ids = big["ids"].to(DEV)
    partials = torch.full((lib.sd_grad_sumsq_workspace_bytes(n) // 8,), fill, dtype=torch.float64, device=DEV)
    table = build_table(lib, big["slots"], n) if kind == "lamb" else None
    ws = torch.full((2 * table[2],), fill, dtype=torch.float64, device=DEV) if table else None
    for t, gr in enumerate(big["grads"], 1):
        gr = gr.to(DEV)
        if poison == t:
            gr[n // 3] = float("inf")
        kw = dict(wd=WD, max_norm=f32(1.0), ema=ema, ema_decay=f32(0.9), status=status, partials=partials)
        if kind == "lamb":
            lamb_step(lib, p, gr, m, v, t, ids, [1.0], [1.0], table, ws=ws, **kw)
        else:
            sgd_step(lib, p, gr, m, ids, [1.0], [1.0], momentum=f32(0.9), **kw)
    return p, m, v, ema, status


@pytest.mark.parametrize("kind", ["sgd", "lamb"])
def test_same_bits_whatever_the_workspaces_held(big, kind):
    from structuredetector_amd import _lib as L
    lib = L.lib()
    runs = [_big_run(lib, big, kind, fill) for fill in (0.0, float("nan"), 1e300)]
    for other in runs[1:]:
        for name, a, b in zip(("param", "state 1", "state 2", "ema", "status"), runs[0], other):
            assert torch.equal(a, b), f"{kind}: {name} depends on what the workspace held"
    assert not torch.equal(runs[0][0].cpu(), big["p0"]) and read_status(runs[0][4])[2] == 0
    if kind == "lamb":                               # the slot larger than a sweep is also right
        n, slots = big["n"], big["slots"]
        one = torch.ones(n, dtype=torch.float64)
        refs = []
        for dtype in (torch.float64, torch.float32):
            p, m, v = big["p0"], torch.zeros(n), torch.zeros(n)
            for t, gr in enumerate(big["grads"], 1):
                p, m, v = lamb_reference_step(dtype, p, gr, m, v, t, slots, one * LR_LAMB, one * WD, f32(1.0))
            refs.append((p, m, v))
        for name, a, w, y in zip(("param", "exp_avg", "exp_avg_sq"), runs[0], *refs):
            close(f"big slot {name}", a, w, y)


@pytest.mark.parametrize("kind", ["sgd", "lamb"])
def test_a_non_finite_gradient_skips_the_whole_step_and_the_next_one_proceeds(big, kind):
    from structuredetector_amd import _lib as L
    lib = L.lib()
    n = big["n"]
    p, m, v, ema, status = _big_run(lib, dict(big, grads=big["grads"][:1]), kind, 0.0, poison=1)
    norm, coef, skipped = read_status(status)
    assert not np.isfinite(norm) and coef == 0.0 and skipped == 1
    assert torch.equal(p.cpu(), big["p0"]) and torch.equal(ema.cpu(), big["p0"]) and not bool(m.any()) and not bool(v.any())
    # the same buffers, a finite gradient: the step runs and the count stays
    ids = big["ids"].to(DEV)
    kw = dict(wd=WD, max_norm=f32(1.0), ema=ema, ema_decay=f32(0.9), status=status)
    if kind == "lamb":
        lamb_step(lib, p, big["grads"][1].to(DEV), m, v, 1, ids, [1.0], [1.0], build_table(lib, big["slots"], n), **kw)
    else:
        sgd_step(lib, p, big["grads"][1].to(DEV), m, ids, [1.0], [1.0], momentum=f32(0.9), **kw)
    norm, coef, skipped = read_status(status)
    assert np.isfinite(norm) and 0 < coef <= 1 and skipped == 1
    assert float((p.cpu() != big["p0"]).float().mean()) > 0.99 and bool(m.any())


def test_lamb_clamps_a_table_that_ends_past_the_buffer(data):
    """The table is laid out for a buffer 64 floats longer than the one the step is told about: the kernels clamp the last slot's range
    to n, and the 64 guard floats behind every buffer keep their bits.  (Not a provoked fault: the clamp is the contract.)"""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    n, guard = data["n"], 64
    slots = data["slots"][:-1] + [(data["slots"][-1][0], n + guard, True)]
    table = build_table(lib, slots, n + guard)
    g = torch.Generator().manual_seed(8)
    bufs = [torch.randn(n + guard, generator=g).to(DEV) for _ in range(2)] + [torch.rand(n + guard, generator=g).to(DEV) * 1e-4] + \
           [torch.randn(n + guard, generator=g).to(DEV)]
    p, m, v, ema = bufs
    before = [b.clone() for b in bufs]
    gr = (torch.randn(n + guard, generator=g) * 0.02).to(DEV)
    ids = torch.zeros((n + guard) // 4, dtype=torch.uint8, device=DEV)
    lamb_step(lib, p, gr, m, v, 2, ids, [1.0], [1.0], table, wd=WD, max_norm=f32(1.0), ema=ema, ema_decay=f32(0.9), status=new_status(), n=n)
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "ema"), bufs, before):
        assert torch.equal(a[n:], b[n:]), f"{name}: the floats behind the buffer changed"
        assert float((a[:n] != b[:n]).float().mean()) > 0.99, f"{name}: the buffer itself was updated"


# ---- TrainStep -----------------------------------------------------------------------------------------------------------------------------
KINDS = {"sgd": dict(optimizer="sgd", momentum=0.9, nesterov=True), "lamb": dict(optimizer="lamb")}
STEP_OPTIONS = dict(weight_decay=0.05, clip_grad_norm=0.5, ema_decay=0.9)


def _net_tables(net, step):
    """The real slot table and per-element rates of the network behind the step's frozen prefix, from `_flat_order` / `_flat_off`."""
    off = step.frozen_off
    ids, groups = net.optim_groups()
    elem_ids = ids.repeat_interleave(4).long()[off:]
    slots = []
    for p in net._flat_order:
        lo, count = net._flat_off[id(p)]
        if lo >= off:
            slots.append((lo - off, lo - off + (count + 7) // 8 * 8, p.dim() == 4))
    mults = step.lr_mults or {}
    lr_mul = [f32(mults.get(stage, 1.0)) for stage, _ in groups]
    wds = [f32mul(step.weight_decay, float(decayed)) for _, decayed in groups]
    return off, elem_ids, slots, lr_mul, wds


def _check_train_steps(kind, net, step, batches, calls, accum=1):
    """`calls` optimizer steps; after each, the parameters the fp64 reference gives from the parameters before the step and the
    gradient the step left in `flat_grads` (the sum over `accum` micro-batches: the reference is fed the mean)."""
    off, elem_ids, slots, lr_mul, wds = _net_tables(net, step)
    n = net.flat_params.numel() - off
    max_norm = f32(step.clip_grad_norm)
    sgd = m = v = None
    if kind == "lamb":
        m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, calls + 1):
        before = net.flat_params.detach().cpu().clone()
        lr = f32(step.lr)
        for k in range(accum):
            step(*batches[(t * accum + k) % 2])
            assert step.updated == (k == accum - 1)
        torch.cuda.synchronize()
        grad = net.flat_grads.detach().cpu().double()[off:] / accum
        lrs = [f32mul(lr, x) for x in lr_mul]
        if kind == "sgd":
            if sgd is None:
                sgd = TorchSgd(torch.float64, before[off:], elem_ids, lrs, wds, f32(step.momentum), step.nesterov)
            want = sgd.step(grad, max_norm, start=before[off:])
            state = {"momentum_buf": (step.exp_avg, sgd.momentum_buffer())}
        else:
            lr_elem, wd_elem = torch.tensor(lrs, dtype=torch.float64)[elem_ids], torch.tensor(wds, dtype=torch.float64)[elem_ids]
            want, m, v = lamb_reference_step(torch.float64, before[off:], grad, m, v, t, slots, lr_elem, wd_elem, max_norm)
            state = {"exp_avg": (step.exp_avg, m), "exp_avg_sq": (step.exp_avg_sq, v)}
        close(f"{kind} step {t} param", net.flat_params[off:], want)
        for name, (got, ref) in state.items():
            close(f"{kind} step {t} {name}", got[off:], ref)
        assert torch.equal(net.flat_params[:off].cpu(), before[:off])
    assert int(step.skipped_steps) == 0 and step.step_count == calls


@pytest.mark.parametrize("kind", ["sgd", "lamb"])
def test_train_step_calls_the_new_entry_point_and_matches_the_reference(kind, monkeypatch):
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model.trainer import TrainStep
    args, net, batches = _small_step_setup(seed=21)
    real = L.lib()
    step = TrainStep(net, args, **KINDS[kind])       # no option on: still the groups form, a uniform table
    assert (step.exp_avg_sq is None) == (kind == "sgd") and step.group_ids is not None and list(step._lr_mul) == [1.0] * 14
    spy = _Spy(real)
    monkeypatch.setattr(L, "_lib", spy)
    step(*batches[0])
    torch.cuda.synchronize()
    monkeypatch.setattr(L, "_lib", real)
    called = set(spy.calls)
    assert f"sd_{kind}_step" in called and not called & {"sd_adam_step", "sd_optim_step", "sd_optim_groups_step", "sd_grad_sumsq"}, sorted(called)
    # two steps with every option on, against the reference on the network's real slot table
    args, net, batches = _small_step_setup(seed=22)
    step = TrainStep(net, args, lr_mults={"adpater": 0.5, "head": 2.0}, **KINDS[kind], **STEP_OPTIONS)
    spy = _Spy(real)
    monkeypatch.setattr(L, "_lib", spy)
    _check_train_steps(kind, net, step, batches, 2)
    monkeypatch.setattr(L, "_lib", real)
    called = set(spy.calls)
    assert {f"sd_{kind}_step", "sd_grad_sumsq"} <= called and not called & {"sd_adam_step", "sd_optim_step", "sd_optim_groups_step"}
    assert not torch.equal(step.ema, net.flat_params)


@pytest.mark.parametrize("kind", ["sgd", "lamb"])
def test_train_step_behind_a_frozen_prefix_and_with_accumulation(kind):
    from structuredetector_amd.model.trainer import TrainStep
    args, net, batches = _small_step_setup(seed=23)
    net.freeze(2)
    p0 = net.flat_params.detach().clone()
    step = TrainStep(net, args, accum_steps=2, **KINDS[kind], **STEP_OPTIONS)
    off = step.frozen_off
    assert off > 0 and off == net.frozen_range()[1]
    _check_train_steps(kind, net, step, batches, 2, accum=2)
    assert torch.equal(net.flat_params[:off], p0[:off]) and torch.equal(step.ema[:off], p0[:off]) and not bool(step.exp_avg[:off].any())
    assert float((net.flat_params[off:] != p0[off:]).float().mean()) > 0.8


@pytest.mark.parametrize("kind", ["sgd", "lamb"])
def test_resume_gives_the_bits_of_the_uninterrupted_run_and_refuses_another_kind(kind, tmp_path):
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    args, net, batches = _small_step_setup(seed=24)
    step = TrainStep(net, args, **KINDS[kind], **STEP_OPTIONS)
    for k in range(3):
        step(*batches[k % 2])
    args2, net2, _ = _small_step_setup(seed=24)
    step2 = TrainStep(net2, args2, **KINDS[kind], **STEP_OPTIONS)
    for k in range(2):
        step2(*batches[k % 2])
    state = step2.state_dict()
    assert state["optimizer"] == kind and ("exp_avg_sq" in state) == (kind == "lamb")
    assert (state["momentum"], state["nesterov"]) == (0.9, kind == "sgd")
    torch.save({"model": {k: v.detach().cpu().clone() for k, v in net2.state_dict().items()}, "optimizer": state}, tmp_path / "resume.pth")
    state = torch.load(tmp_path / "resume.pth", map_location="cpu", weights_only=True)
    net3 = Network(args2, pretrained=False).to(args2.device).train()
    net3.load_state_dict(state["model"])
    step3 = TrainStep(net3, args2, **KINDS[kind])
    step3.load_state_dict(state["optimizer"])
    step3(*batches[0])
    torch.cuda.synchronize()
    assert torch.equal(net3.flat_params, net.flat_params), "resumed run diverged from the uninterrupted one"
    assert torch.equal(step3.exp_avg, step.exp_avg) and torch.equal(step3.ema, step.ema)
    assert step3.exp_avg_sq is None if kind == "sgd" else torch.equal(step3.exp_avg_sq, step.exp_avg_sq)
    # across kinds: refused, naming both
    other = "lamb" if kind == "sgd" else "sgd"
    with pytest.raises(L.SdError, match=rf"(?s)'{kind}'.*'{other}'"):
        TrainStep(net3, args2, **KINDS[other]).load_state_dict(state["optimizer"])
    with pytest.raises(L.SdError, match=rf"(?s)'{kind}'.*'adam'"):
        TrainStep(net3, args2).load_state_dict(state["optimizer"])
    adam_state = TrainStep(net3, args2).state_dict()
    assert "optimizer" not in adam_state and "momentum" not in adam_state and "nesterov" not in adam_state
    with pytest.raises(L.SdError, match=rf"(?s)'adam'.*'{kind}'"):
        step3.load_state_dict(adam_state)            # a state without the key is Adam's


# ---- command line ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, kind", [(["--optimizer", "lamb", "--weight_decay", "0.01", "--clip_grad_norm", "1"], "lamb"),
                                         (["--optimizer", "sgd", "--nesterov"], "sgd")])
def test_train_cli_runs_and_writes_a_resumable_checkpoint(flags, kind, tmp_path, monkeypatch, capsys):
    from structuredetector_amd.cli import train
    from structuredetector_amd.model.trainer import Trainer
    from structuredetector_amd.utils.args import Arguments
    monkeypatch.chdir(tmp_path)
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    common = ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "--synthetic", "8", "-b", "4", "-e", "1", "--steps", "2"]
    train.main(common + flags)
    out = capsys.readouterr().out
    assert "update rule: " + ("LAMB" if kind == "lamb" else "SGD, momentum 0.9 (Nesterov)") in out and "epoch 0: total" in out
    resume = list((tmp_path / "trainings").glob("*/resume.pth"))
    assert len(resume) == 1
    state = torch.load(resume[0], map_location="cpu", weights_only=True)
    assert state["optimizer"]["optimizer"] == kind and state["optimizer"]["step_count"] == 2
    assert ("exp_avg_sq" in state["optimizer"]) == (kind == "lamb")
    tr = Trainer(Arguments().parse(common + flags + ["--resume", str(resume[0])]))
    assert tr.step.optimizer == kind and tr.step.step_count == 2 and bool(tr.step.exp_avg.any())
    from structuredetector_amd import _lib as L
    with pytest.raises(L.SdError, match="optimizer"):
        Trainer(Arguments().parse(common + ["--resume", str(resume[0])]))
