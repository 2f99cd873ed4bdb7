"""Per-group learning rates on the GPU: `sd_optim_groups_step` against `sd_optim_step` (bit for bit where the table is uniform) and against
torch.optim.AdamW with one param group per id, `TrainStep(lr_mults=...)` on the small net, and the Trainer with warm-up + cosine through a
resume.  Shapes, tolerance and the fp32 hyper-parameters are those of tests/test_gpu_optim.py; expected values come from torch and from
formulas written out here, never from the code under test."""
import ctypes as C
import json
import math
import shutil

import numpy as np
import pytest
import torch

from tests.test_gpu_optim import ADAM_TOL, B1, B2, EPS, LR, N_TAIL, _small_step_setup, _Spy, f32, new_status, optim_step, read_status, sumsq

pytestmark = pytest.mark.gpu
DEV = "cuda"


def floats(values):
    return (C.c_float * len(values))(*values)


def groups_step(lib, p, g, m, v, step, ids, lr_mul, wd_mul, lr=LR, gscale=1.0, wd=0.0, max_norm=0.0, ema=None, ema_decay=0.0, status=None):
    from structuredetector_amd import _lib as L
    partials = sumsq(lib, g) if max_norm > 0 else None
    L.check(lib.sd_optim_groups_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step, lr, B1, B2, EPS, gscale, wd,
                                     ids.data_ptr(), floats(lr_mul), floats(wd_mul), len(lr_mul), max_norm,
                                     None if partials is None else partials.data_ptr(), 0 if partials is None else partials.numel(),
                                     None if ema is None else ema.data_ptr(), ema_decay, None if status is None else status.data_ptr(),
                                     L.stream()), "sd_optim_groups_step")
    torch.cuda.synchronize()


@pytest.mark.parametrize("options", ["all", "no_clip", "no_ema"])
@pytest.mark.parametrize("n", [1000, 4096, N_TAIL])
def test_uniform_table_is_optim_step_bit_for_bit(n, options):
    """ids = the 0 / 1 decay mask, lr_mul = [1, 1], wd_mul = [0, 1]: the launch must leave sd_optim_step's bits in every buffer."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    wd, gscale = f32(0.05), 0.5
    max_norm = 0.0 if options == "no_clip" else f32(0.3)
    with_ema = options != "no_ema"
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    mask = (torch.rand(n // 4, generator=g) < 0.6).to(torch.uint8).to(DEV)
    grads = [(torch.randn(n, generator=g) * 0.05).to(DEV) for _ in range(3)]
    decays = [f32(min(0.99, (1 + t) / (10 + t))) for t in range(1, 4)]
    runs = []
    for grouped in (False, True):
        p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        ema, status = (p0.to(DEV) if with_ema else None), new_status()
        for step, (gr, d) in enumerate(zip(grads, decays), 1):
            kw = dict(gscale=gscale, wd=wd, max_norm=max_norm, ema=ema, ema_decay=d if with_ema else 0.0, status=status)
            if grouped:
                groups_step(lib, p, gr, m, v, step, mask, [1.0, 1.0], [0.0, 1.0], **kw)
            else:
                optim_step(lib, p, gr, m, v, step, mask=mask, **kw)
        runs.append((p, m, v, status) + ((ema,) if with_ema else ()))
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "status", "ema"), *runs):
        assert torch.equal(a, b), f"{name} differs from sd_optim_step"
    assert not torch.equal(runs[1][0].cpu(), p0)
    if max_norm:
        norm, coef, skipped = read_status(runs[1][3])
        assert norm > max_norm and 0 < coef < 1 and skipped == 0            # the clipped path ran


def test_uniform_table_is_optim_step_over_many_rates_and_step_numbers():
    """The grouped entry point divides lr / bc1 on the host, sd_optim_step's kernel on the device: the same bits for rates from 1e-6 to 0.3
    and bias corrections from step 1 to step 50 000 (bc1 from 0.1 to 1)."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    n, wd = 4096, f32(0.05)
    g = torch.Generator().manual_seed(77)
    p0 = torch.randn(n, generator=g)
    mask = (torch.rand(n // 4, generator=g) < 0.5).to(torch.uint8).to(DEV)
    cases = [(step, f32(lr)) for step in (1, 2, 3, 5, 11, 37, 150, 1000, 50_000) for lr in (1e-6, 3.3e-5, 1e-3, 7.7e-3, 0.3)]
    grads = (torch.randn(n, generator=g) * 0.05).to(DEV)
    state = [[p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)] for _ in range(2)]
    for step, lr in cases:
        p, m, v = state[0]
        L.check(lib.sd_optim_step(p.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, lr, B1, B2, EPS, 1.0, wd, mask.data_ptr(), 0.0,
                                  None, 0, None, 0.0, None, L.stream()), "sd_optim_step")
        p, m, v = state[1]
        groups_step(lib, p, grads, m, v, step, mask, [1.0, 1.0], [0.0, 1.0], lr=lr, wd=wd)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), *state):
            assert torch.equal(a, b), f"{name} differs from sd_optim_step at step {step}, lr {lr}"
    assert not torch.equal(state[1][0].cpu(), p0)


def _torch_groups(dtype, p0, grads, elem_ids, lrs, wds, max_norm, ema_decays=None):
    """torch.optim.AdamW with one param group per id (`lrs[step][k]`, `wds[k]`), clip_grad_norm_ over all groups before each step, the
    EMA recurrence written out.  Returns flat parameters, both moments and the EMA."""
    sel = [(elem_ids == k).nonzero().squeeze(1) for k in range(len(wds))]
    params = [p0[s].to(dtype).clone().requires_grad_(True) for s in sel]
    opt = torch.optim.AdamW([dict(params=[q], lr=lrs[0][k], weight_decay=wds[k]) for k, q in enumerate(params)], lr=1.0, betas=(B1, B2), eps=EPS)
    ema = p0.to(dtype).clone()

    def flat(parts):
        out = torch.zeros(p0.numel(), dtype=dtype)
        for s, part in zip(sel, parts):
            out[s] = part
        return out

    for t, gr in enumerate(grads):
        gr = gr.to(dtype)
        for k, (group, q) in enumerate(zip(opt.param_groups, params)):
            group["lr"] = lrs[t][k]
            q.grad = gr[sel[k]].clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        if ema_decays is not None:
            ema = ema_decays[t] * ema + (1 - ema_decays[t]) * flat([q.detach() for q in params])
    return (flat([q.detach() for q in params]), flat([opt.state[q]["exp_avg"] for q in params]),
            flat([opt.state[q]["exp_avg_sq"] for q in params]), ema)


def _group_lr(lr, mult):
    """lr_k as the entry point forms it: one fp32 multiply of the fp32 arguments."""
    return float(np.float32(lr) * np.float32(mult))


def test_sixteen_random_groups_against_torch_adamw_with_sixteen_param_groups():
    """Truth: torch in fp64; torch's own fp32 run is printed beside each figure (`pytest -s`).  Bound, per buffer: ADAM_TOL = 1e-6 of the
    largest value.  Ids are drawn per float4, so group boundaries fall inside waves and blocks; the rate changes every step (the five
    warm-up values of N = 5)."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    n, wd, gscale = N_TAIL, f32(0.05), 0.5
    g = torch.Generator().manual_seed(16)
    p0 = torch.randn(n, generator=g)
    ids = torch.randint(0, 16, (n // 4,), generator=g, dtype=torch.uint8)
    elem_ids = ids.repeat_interleave(4).long()
    choices = [0.0, 0.01, 0.1, 0.5, 1.0, 2.0]
    lr_mul = [f32(choices[int(c)]) for c in torch.randint(0, 6, (16,), generator=g)]
    wd_mul = [float(b) for b in torch.randint(0, 2, (16,), generator=g)]
    lr_mul[3], wd_mul[3], lr_mul[8], wd_mul[8] = 0.0, 1.0, 0.0, 0.0          # a group that stands still, with and without decay
    assert all(int((ids == k).sum()) > 0 for k in range(16))
    grads = [torch.randn(n, generator=g) * 0.02 for _ in range(5)]          # the averaged gradients; the kernel is fed 2 x with grad_scale 0.5
    max_norm = f32(0.5 * float(grads[0].double().norm()))
    lrs = [f32(1e-3 * ((i + 1) / 5)) for i in range(5)]
    ema_decays = [f32(min(0.99, (1 + t) / (10 + t))) for t in range(1, 6)]
    group_lrs = [[_group_lr(lr, mult) for mult in lr_mul] for lr in lrs]
    group_wds = [wd * w for w in wd_mul]
    want = _torch_groups(torch.float64, p0, grads, elem_ids, group_lrs, group_wds, max_norm, ema_decays)
    yard = _torch_groups(torch.float32, p0, grads, elem_ids, group_lrs, group_wds, max_norm, ema_decays)
    p, m, v, ema, status = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(DEV), new_status()
    for step, (gr, lr, d) in enumerate(zip(grads, lrs, ema_decays), 1):
        groups_step(lib, p, (gr * 2).to(DEV), m, v, step, ids.to(DEV), lr_mul, wd_mul, lr=lr, gscale=gscale, wd=wd, max_norm=max_norm, ema=ema,
                    ema_decay=d, status=status)
        norm, coef, skipped = read_status(status)
        assert 0 < coef < 1 and skipped == 0
    got = (p.cpu(), m.cpu(), v.cpu(), ema.cpu())
    for name, a, w, y in zip(("param", "exp_avg", "exp_avg_sq", "ema"), got, want, yard):
        scale = w.abs().max().item()
        err, err32 = (a.double() - w).abs().max().item(), (y.double() - w).abs().max().item()
        print(f"{name}: err/scale {err / scale:.3e}, torch fp32 err/scale {err32 / scale:.3e}")
        assert err <= ADAM_TOL * scale, f"{name}: {err:.3e} vs fp64, torch fp32 {err32:.3e}, scale {scale:.3e}"
    for k in (3, 8):                             # lr_k = 0: decay_mul = 1 whatever wd_mul says -- the parameter keeps its start value
        still = elem_ids == k
        assert torch.equal(got[0][still], p0[still])
        assert float(got[1][still].abs().max()) > 0 and float(got[2][still].abs().max()) > 0, "the moments of an lr = 0 group still update"
    moved = elem_ids == next(k for k in range(16) if lr_mul[k] > 0)
    assert not torch.equal(got[0][moved], p0[moved])


def test_one_group_a_stray_id_and_a_skipped_step():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    n, wd = 256 * 4 * 9 + 8, f32(0.05)
    g = torch.Generator().manual_seed(5)
    p0, m0, v0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-4
    e0 = torch.randn(n, generator=g)
    gr = (torch.randn(n, generator=g) * 0.1).to(DEV)
    kw = dict(wd=wd, max_norm=1.0, ema_decay=0.9)

    def start():
        return p0.to(DEV), m0.to(DEV), v0.to(DEV), e0.to(DEV), new_status()

    # ngroups = 1: sd_optim_step without a mask (everything decayed)
    pa, ma, va, ea, sa = start()
    optim_step(lib, pa, gr, ma, va, 3, ema=ea, status=sa, **kw)
    pb, mb, vb, eb, sb = start()
    groups_step(lib, pb, gr, mb, vb, 3, torch.zeros(n // 4, dtype=torch.uint8, device=DEV), [1.0], [1.0], ema=eb, status=sb, **kw)
    for a, b in ((pa, pb), (ma, mb), (va, vb), (ea, eb), (sa, sb)):
        assert torch.equal(a, b)
    # ngroups = 3 and one id byte of 200: 200 & 15 = 8 >= 3 names a row that does not move
    ids = torch.randint(0, 3, (n // 4,), generator=g, dtype=torch.uint8)
    j = n // 8 + 3
    ids[j] = 200
    p, m, v, ema, status = start()
    groups_step(lib, p, gr, m, v, 3, ids.to(DEV), [1.0, 0.5, 2.0], [1.0, 0.0, 1.0], ema=ema, status=status, **kw)
    p = p.cpu()
    assert torch.equal(p[4 * j:4 * j + 4], p0[4 * j:4 * j + 4])
    changed = (p != p0).view(-1, 4).any(dim=1)
    changed[j] = True
    assert bool(changed.all()), "every other group of four moved"
    # a non-finite gradient skips the step for every group
    poisoned = gr.clone()
    poisoned[n // 3] = float("inf")
    p, m, v, ema, status = start()
    groups_step(lib, p, poisoned, m, v, 3, ids.to(DEV), [1.0, 0.5, 2.0], [1.0, 0.0, 1.0], ema=ema, status=status, **kw)
    norm, coef, skipped = read_status(status)
    assert not np.isfinite(norm) and coef == 0.0 and skipped == 1
    for held, first in ((p, p0), (m, m0), (v, v0), (ema, e0)):
        assert torch.equal(held.cpu(), first)


def test_train_step_with_lr_mults_calls_the_grouped_entry_point_and_matches_torch(monkeypatch):
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model.trainer import TrainStep
    from structuredetector_amd.utils.args import stage_lr_mults
    mults = stage_lr_mults(0.1, 0.5)
    args, net, batches = _small_step_setup(seed=4)
    real = L.lib()
    for kw, want, never in ((dict(lr_mults=mults), {"sd_optim_groups_step"}, {"sd_optim_step", "sd_adam_step", "sd_grad_sumsq"}),
                            (dict(lr_mults=mults, clip_grad_norm=1.0), {"sd_optim_groups_step", "sd_grad_sumsq"}, {"sd_optim_step", "sd_adam_step"}),
                            ({}, {"sd_adam_step"}, {"sd_optim_step", "sd_optim_groups_step"}),
                            (dict(weight_decay=0.01), {"sd_optim_step"}, {"sd_adam_step", "sd_optim_groups_step"})):
        step = TrainStep(net, args, **kw)
        spy = _Spy(real)
        monkeypatch.setattr(L, "_lib", spy)
        step(*batches[0])
        torch.cuda.synchronize()
        monkeypatch.setattr(L, "_lib", real)
        called = set(spy.calls)
        assert want <= called and not (never & called), (kw, sorted(called))
    # three steps against torch.optim.AdamW in fp64 over the 14 groups of optim_groups(), fed the step's own gradients
    args, net, batches = _small_step_setup(seed=4)
    wd, max_norm = 0.05, 0.5
    step = TrainStep(net, args, lr_mults=mults, weight_decay=wd, clip_grad_norm=max_norm)
    ids, groups = net.optim_groups()
    assert torch.equal(step.group_ids.cpu(), ids) and step.decay_mask is None
    elem_ids = ids.repeat_interleave(4).long()
    p0 = net.flat_params.detach().cpu().clone()
    rates, grads = [1e-3, 5e-4, 2e-3], []
    for k, lr in enumerate(rates):
        step.lr = lr                                   # what the schedule does before every step
        step(*batches[k % 2])
        torch.cuda.synchronize()
        grads.append(net.flat_grads.detach().cpu().clone())
    assert int(step.skipped_steps) == 0
    lrs = [[_group_lr(f32(lr), f32(mults[stage])) for stage, _ in groups] for lr in rates]
    wds = [f32(wd) * float(decayed) for _, decayed in groups]
    want = _torch_groups(torch.float64, p0, grads, elem_ids, lrs, wds, f32(max_norm))
    for name, a, w in zip(("param", "exp_avg", "exp_avg_sq"), (net.flat_params, step.exp_avg, step.exp_avg_sq), want):
        scale = w.abs().max().item()
        err = (a.detach().cpu().double() - w).abs().max().item()
        print(f"train step {name}: err/scale {err / scale:.3e}")
        assert err <= ADAM_TOL * scale, f"{name}: {err:.3e} vs fp64, scale {scale:.3e}"
    # the stem moved 0.1 * 0.5 ** 5 as far as it would at the head's rate: far less than the head
    stem = elem_ids == 1
    head = elem_ids == 13
    final = net.flat_params.detach().cpu()
    assert 0 < float((final - p0)[stem].abs().max()) < 0.05 * float((final - p0)[head].abs().max())


def test_train_step_with_lr_mults_leaves_the_frozen_prefix_alone():
    from structuredetector_amd.model.trainer import TrainStep
    from structuredetector_amd.utils.args import stage_lr_mults
    args, net, batches = _small_step_setup(seed=6)
    net.freeze(2)
    step = TrainStep(net, args, lr_mults=stage_lr_mults(0.1, 0.5), weight_decay=0.05, clip_grad_norm=0.5, ema_decay=0.9)
    off = step.frozen_off
    assert off > 0 and off == net.frozen_range()[1]
    p0 = net.flat_params.detach().clone()
    for k in range(3):
        step(*batches[k % 2])
    torch.cuda.synchronize()
    assert int(step.skipped_steps) == 0
    assert torch.equal(net.flat_params[:off], p0[:off]) and torch.equal(step.ema[:off], p0[:off])
    assert not bool(step.exp_avg[:off].any()) and not bool(step.exp_avg_sq[:off].any())
    ids = step.group_ids.cpu().repeat_interleave(4)
    assert int(ids[off]) // 2 == 2 and int(ids[:off].max()) // 2 == 1        # the suffix starts with down2's groups
    moved = net.flat_params[off:] != p0[off:]
    assert float(moved.float().mean()) > 0.8


def _formula(i, base=1e-3, n=3, t=6, min_lr=0.0):
    if i < n:
        return base * ((i + 1) / n)
    return min_lr + (base - min_lr) * 0.5 * (1 + math.cos(math.pi * (i - n) / (t - n))) if i < t else min_lr


def test_trainer_warm_up_cosine_and_backbone_multiplier_through_a_resume(tmp_path, monkeypatch, capsys):
    from structuredetector_amd.model.trainer import Trainer, TrainStep
    from structuredetector_amd.utils.args import Arguments
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    monkeypatch.chdir(tmp_path)
    argv = ["-s", "stem", "--labels", str(tmp_path / "labels.json"), "--synthetic", "8", "--steps", "6", "--epochs", "2", "-b", "2", "-W", "128",
            "-H", "128", "--warmup_steps", "3", "--lr_schedule", "cosine", "--backbone_lr_mult", "0.1"]
    seen, names = [], []
    inner_call = TrainStep.__call__

    def recording(self, images, targets):
        seen.append(self.lr)
        return inner_call(self, images, targets)

    monkeypatch.setattr(TrainStep, "__call__", recording)
    tr = Trainer(Arguments().parse(argv))
    assert tr.scheduler.total_steps == 6 and tr.scheduler.per_step and tr.step.lr_mults["down4"] == 0.1 and tr.step.lr_mults["fpn"] == 1.0
    inner_save = tr.save_resume

    def keep_first(path):
        inner_save(path)
        if tr.epoch == 0:
            shutil.copy(path, tmp_path / "after_epoch_0.pth")

    monkeypatch.setattr(tr, "save_resume", keep_first)
    tr.train()
    assert tr.step.step_count == 6 and len(seen) == 6
    for i, lr in enumerate(seen):
        assert abs(lr - _formula(i)) <= 1e-15 * 1e-3, (i, lr, _formula(i))
    assert seen[2] == 1e-3 == seen[3] and seen[0] < seen[1] < seen[2] and seen[3] > seen[4] > seen[5] > 0
    out = capsys.readouterr().out
    assert "learning rate: cosine" in out and "warm-up over the first 3 steps" in out and "down4 0.1" in out
    rows = [json.loads(ln) for ln in (tr.save_dir / "scalars.jsonl").read_text().splitlines()]
    assert [r["value"] for r in rows if r["tag"] == "Learning rate"] == seen           # one per step, the values the launches got
    # resume after the first epoch (4 steps) with the same command line: the run ends where the uninterrupted one did
    del seen[:]
    tr2 = Trainer(Arguments().parse(argv + ["--resume", str(tmp_path / "after_epoch_0.pth")]))
    assert tr2.step.step_count == 4 and tr2.start_epoch == 1
    tr2.train()
    assert tr2.step.step_count == 6 and seen == [_formula(4), _formula(5)]
    assert torch.equal(tr2.net.flat_params, tr.net.flat_params)
    assert torch.equal(tr2.step.exp_avg, tr.step.exp_avg) and torch.equal(tr2.step.exp_avg_sq, tr.step.exp_avg_sq)
    # another schedule on the command line than in the file is refused, naming both; other multipliers are named and the command line wins
    capsys.readouterr()
    with pytest.raises(ValueError, match=r"(?s)--warmup_steps 3.*--warmup_steps 2"):
        Trainer(Arguments().parse(argv[:-6] + ["--warmup_steps", "2", "--lr_schedule", "cosine", "--resume", str(tmp_path / "after_epoch_0.pth")]))
    out = capsys.readouterr().out
    assert "per-stage learning-rate multipliers adpater 0.1" in out and "continues with none" in out
    with pytest.raises(ValueError, match="warmup_steps"):
        Trainer(Arguments().parse(argv[:-6] + ["--warmup_steps", "6", "--lr_schedule", "cosine"]))
