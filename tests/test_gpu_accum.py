"""Gradient accumulation on the GPU: `sd_grad_accum` bit for bit against torch's add / copy on the device, and `TrainStep(accum_steps=K)`
through the optimizer variants, `flush()`, frozen stages, the non-finite guard and the Trainer.

Everything here is an equality of bits.  The kernel is one fp32 add per element (the reference: `torch.add` of the same two device
tensors), the accumulator is the fp32 running sum of the gradients the plain backward wrote (the reference: those gradients, snapshot
by snapshot or recomputed on a copy of the network, added with torch in the stated order ((g1 + g2) + g3)), and the optimizer launch is
the one the C ABI gives on the same buffers with grad_scale = 1 / k.  The fp32 step is bit-reproducible, so the recomputation is an
independent check there; the mixed-precision step is documented as not reproducible, so under `--amp` only the self-consistent checks
run."""
import json

import numpy as np
import pytest
import torch

from tests.test_gpu_optim import N_TAIL, _Spy

pytestmark = pytest.mark.gpu
DEV = "cuda"
SD_ERR_INVALID, SD_ERR_ALIGN = -1, -3                                   # include/sdnet_hip.h
OPTIONS = dict(weight_decay=0.05, clip_grad_norm=0.5, ema_decay=0.9)    # tests/test_gpu_freeze.py


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
GUARD = 8            # floats before and after each range that no launch may touch
# One pass of the grid covers 4096 blocks x 256 threads x 4 floats = 4 * 2**20 floats.  3 * 2**20 + 4 is the large case the feature was
# specified with; it still fits one pass, so 4 * 2**20 + 4 stands beside it: the smallest size whose last group is reached only by the
# second trip of the grid-stride loop.
SIZES = [4, 252, 1000, 4096, N_TAIL, 3 * 2 ** 20 + 4, 4 * 2 ** 20 + 4]


def _values(n, seed):
    """Normal values with every special one planted: both zeros, denormals of both signs, the largest finite value (its sum with itself
    overflows), both infinities (inf + -inf is a nan) and a nan."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.tensor([1.0, 1e-3, 1e3, 1e-30])[torch.randint(0, 4, (n,), generator=g)]
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 3.4028234e38, -3.4028234e38, float("inf"), -float("inf"), float("nan")])
    at = torch.randperm(n, generator=g)[:min(n, 3 * special.numel())]
    x[at] = special[torch.arange(at.numel()) % special.numel()]
    return x


@pytest.mark.parametrize("overwrite", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_is_torch_add_or_copy_bit_for_bit(n, overwrite):
    from structuredetector_amd import _lib as L
    lib = L.lib()
    for doff, soff in ((0, 0), (4, 0), (0, 4), (4, 4)):                  # element offsets inside buffers with guard cells on both sides
        a = _values(n, 3 * n + doff).to(DEV)
        b = _values(n, 5 * n + soff + 1).to(DEV)
        if n >= 4:                                                        # the pairings a random draw rarely gives
            a[:4] = torch.tensor([float("inf"), -0.0, 0.0, 3.4028234e38]); b[:4] = torch.tensor([-float("inf"), 0.0, -0.0, 3.4028234e38])
        dst_buf = torch.full((GUARD + doff + n + GUARD,), 7.25, device=DEV)
        src_buf = torch.full((GUARD + soff + n + GUARD,), -3.5, device=DEV)
        dst, src = dst_buf[GUARD + doff:GUARD + doff + n], src_buf[GUARD + soff:GUARD + soff + n]
        dst.copy_(a); src.copy_(b)
        assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
        want = b.clone() if overwrite else torch.add(a, b)
        dst_before, src_before = dst_buf.clone(), src_buf.clone()
        L.check(lib.sd_grad_accum(dst.data_ptr(), src.data_ptr(), n, overwrite, L.stream()), "sd_grad_accum")
        torch.cuda.synchronize()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(dst), nan), (n, overwrite, doff, soff)
        assert torch.equal(bits(dst)[~nan], bits(want)[~nan]), (n, overwrite, doff, soff)
        if overwrite:                                                     # a copy keeps the nan's payload too
            assert same_bits(dst, b)
        else:
            assert int(nan.sum()) >= 1                                    # inf + -inf at the least
        lo, hi = GUARD + doff, GUARD + doff + n
        assert same_bits(dst_buf[:lo], dst_before[:lo]) and same_bits(dst_buf[hi:], dst_before[hi:])
        assert same_bits(src_buf, src_before)                             # the source, guards included, is only read


def test_kernel_same_range_no_launch_at_zero_and_every_refusal():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    err = lambda: lib.sd_last_error().decode()
    n = 1000
    x = _values(n, 11).to(DEV)
    buf = torch.zeros(n + 16, device=DEV)
    d = buf[4:4 + n]
    d.copy_(x)
    # dst and src the same range: x + x; overwrite: x unchanged
    L.check(lib.sd_grad_accum(d.data_ptr(), d.data_ptr(), n, 0, L.stream()))
    want = torch.add(x, x)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(d), nan) and torch.equal(bits(d)[~nan], bits(want)[~nan])
    L.check(lib.sd_grad_accum(d.data_ptr(), d.data_ptr(), n, 1, L.stream()))
    assert torch.equal(bits(d)[~nan], bits(want)[~nan])
    # touching ranges are not overlapping ones
    left, right = buf[0:8], buf[8:16]
    before = right.clone()
    L.check(lib.sd_grad_accum(left.data_ptr(), right.data_ptr(), 8, 1, L.stream()))
    assert same_bits(left, before) and same_bits(right, before)
    # n == 0: success, nothing written (null pointers are fine there)
    held = buf.clone()
    assert lib.sd_grad_accum(d.data_ptr(), d.data_ptr() + 16, 0, 0, L.stream()) == 0
    assert lib.sd_grad_accum(None, None, 0, 1, L.stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(buf, held)
    # the refusals, each with its code; none writes
    p, q = d.data_ptr(), d.data_ptr() + 4 * 2000                          # (q is never read: every case returns before a launch)
    for args, code, word in (((p, q, -4, 0), SD_ERR_INVALID, "n >= 0"), ((p, q, 10, 0), SD_ERR_INVALID, "n % 4 == 0"),
                             ((None, q, 8, 0), SD_ERR_INVALID, "null"), ((p, None, 8, 1), SD_ERR_INVALID, "null"),
                             ((p, q, 8, 2), SD_ERR_INVALID, "overwrite"), ((p, q, 8, -1), SD_ERR_INVALID, "overwrite"),
                             ((p + 4, q, 8, 0), SD_ERR_ALIGN, "aligned"), ((p, q + 8, 8, 1), SD_ERR_ALIGN, "aligned"),
                             ((p, p + 16, 8, 0), SD_ERR_INVALID, "overlap"), ((p + 16, p, 8, 1), SD_ERR_INVALID, "overlap")):
        assert lib.sd_grad_accum(*args, L.stream()) == code and "sd_grad_accum" in err() and word in err(), (args, err())
    torch.cuda.synchronize()
    assert same_bits(buf, held)


# ---- the step -----------------------------------------------------------------------------------------------------------------------------
def _setup(stages=0, bn=False, amp=False, **kw):
    """The small network and step of tests/test_gpu_freeze.py (make_args(2, 1, 20, 40), B = 2, 128 x 128) with a third batch."""
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    from tests.test_gpu_freeze import _step_setup
    args, net, step, batches = _step_setup(stages=stages, bn=bn, **kw)
    step.amp = amp                                                        # (read by every call: what `use_amp` in the namespace sets)
    enc = Encode(args)
    tgt = enc.render(enc.plan(128, 128, *synthetic_batch(np.random.default_rng(102), 2, 128, 128, 2, 1)), net.flat_params.device)
    x = torch.randn(2, 3, 128, 128, device=net.flat_params.device, generator=torch.Generator(net.flat_params.device).manual_seed(202))
    return args, net, step, batches + [(x, tgt)]


def _state(net, step):
    return dict(p=net.flat_params.clone(), m=step.exp_avg.clone(), v=step.exp_avg_sq.clone(), ema=None if step.ema is None else step.ema.clone())


def _unchanged(net, step, s):
    return (same_bits(net.flat_params, s["p"]) and same_bits(step.exp_avg, s["m"]) and same_bits(step.exp_avg_sq, s["v"])
            and (step.ema is None or same_bits(step.ema, s["ema"])))


def _replay(step, s, grad, k, t):
    """The optimizer launch of update number t through the C ABI, from the saved state `s` on `grad` with grad_scale = 1 / k: the entry
    point the step's options select, called here with the step's own tables.  Returns (param, exp_avg, exp_avg_sq, ema, status)."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    p, m, v = s["p"].clone(), s["m"].clone(), s["v"].clone()
    ema = None if s["ema"] is None else s["ema"].clone()
    n, scale = p.numel(), 1.0 / k
    status = torch.zeros(4, dtype=torch.int32, device=p.device)
    status.view(torch.float32)[1] = 1.0
    clip = step.clip_grad_norm > 0
    partials = None
    if clip:
        partials = torch.empty(lib.sd_grad_sumsq_workspace_bytes(n) // 8, dtype=torch.float64, device=p.device)
        L.check(lib.sd_grad_sumsq(grad.data_ptr(), n, partials.data_ptr(), partials.numel() * 8, L.stream()), "sd_grad_sumsq")
    tail = (step.clip_grad_norm, partials.data_ptr() if clip else None, partials.numel() if clip else 0, None if ema is None else ema.data_ptr(),
            step.ema_decay_at(t) if ema is not None else 0.0, status.data_ptr(), L.stream())
    head = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, t, step.lr, step.betas[0], step.betas[1], step.eps, scale)
    if step.lr_mults is not None:
        L.check(lib.sd_optim_groups_step(*head, step.weight_decay, step.group_ids.data_ptr(), step._lr_mul, step._wd_mul, len(step.groups), *tail),
                "sd_optim_groups_step")
    elif step.plain_adam:
        L.check(lib.sd_adam_step(*head, L.stream()), "sd_adam_step")
    else:
        L.check(lib.sd_optim_step(*head, step.weight_decay, None if step.decay_mask is None else step.decay_mask.data_ptr(), *tail), "sd_optim_step")
    torch.cuda.synchronize()
    return p, m, v, ema, status


def _lr_mults():
    from structuredetector_amd.utils.args import stage_lr_mults
    return stage_lr_mults(0.1, 0.5)


@pytest.mark.parametrize("amp, kw", [(False, {}), (False, OPTIONS), (True, {}), (True, OPTIONS), (False, dict(OPTIONS, lr_mults="stages"))],
                         ids=["fp32-plain", "fp32-options", "amp-plain", "amp-options", "fp32-lr_mults"])
def test_three_micro_steps_accumulate_the_plain_gradients_and_update_once(amp, kw):
    kw = dict(kw, lr_mults=_lr_mults()) if "lr_mults" in kw else dict(kw)
    args, net, step, batches = _setup(amp=amp, accum_steps=3, **kw)
    assert step.accum_steps == 3 and step.micro == 0 and step.updated is False
    assert step.grad_acc.shape == net.flat_grads.shape and step.grad_acc.dtype == torch.float32 and not bool(step.grad_acc.any())
    s0 = _state(net, step)
    running = None
    for j in (1, 2):
        loss = step(*batches[j - 1])
        torch.cuda.synchronize()
        assert loss.shape == (4,) and bool(torch.isfinite(loss).all())
        g = net.flat_grads.clone()                                        # g_j: what the plain backward wrote
        assert bool(g.any())
        running = g if running is None else torch.add(running, g)
        assert same_bits(step.grad_acc, running), j
        assert step.updated is False and step.micro == j and step.step_count == 0 and _unchanged(net, step, s0), j
    step(*batches[2])
    torch.cuda.synchronize()
    assert step.updated is True and step.micro == 0 and step.step_count == 1
    assert same_bits(step.grad_acc, running)                              # the last micro-step reads the accumulator, it does not write it
    total = net.flat_grads.clone()
    assert not same_bits(total, running) and bool(torch.isfinite(total).all())
    p, m, v, ema, status = _replay(step, s0, total, 3, 1)
    assert same_bits(net.flat_params, p) and same_bits(step.exp_avg, m) and same_bits(step.exp_avg_sq, v)
    assert not same_bits(net.flat_params, s0["p"])
    if step.ema is not None:
        assert same_bits(step.ema, ema) and not same_bits(step.ema, s0["ema"])
    if step.clip_grad_norm > 0:
        assert same_bits(step._status[:2], status[:2]) and int(step.skipped_steps) == 0
        want = float(total.double().norm()) / 3                           # the norm of the MEAN gradient
        assert abs(float(step.grad_norm) - want) <= 1e-6 * want
    # the next group starts over: micro-step 1 overwrites the accumulator
    step(*batches[1])
    torch.cuda.synchronize()
    assert step.updated is False and step.micro == 1 and step.step_count == 1 and same_bits(step.grad_acc, net.flat_grads)


def _plain_gradient(args, net, batch):
    """forward_train / loss / backward_from, the pieces the step is made of, called one by one: the batch's gradient in `flat_grads`."""
    from structuredetector_amd.model.loss import loss_backward, loss_config, loss_forward
    x, tgt = batch
    head, tape = net.forward_train(x)
    cfg = loss_config(args, net.label_count, net.part_count, tgt["anchor_inds"].shape[1], tgt["part_inds"].shape[1])
    desc, keep, out8 = loss_forward(head, tgt, cfg)
    dhead = loss_backward(desc, out8, torch.ones((), device=head.device), tuple(head.shape))
    net.backward_from(tape, dhead)
    torch.cuda.synchronize()
    return net.flat_grads.clone()


def test_fp32_total_is_the_sum_of_three_separately_computed_gradients_in_the_stated_order():
    args, net, step, batches = _setup(accum_steps=3)
    for k in range(3):
        step(*batches[k])
    torch.cuda.synchronize()
    assert step.updated and step.step_count == 1
    # a copy of the network (same seed, same construction), never stepped: the weights the three micro-steps saw
    args_b, net_b, _, _ = _setup()
    g1, g2, g3 = (_plain_gradient(args_b, net_b, batches[k]) for k in range(3))
    assert not same_bits(g1, g2) and not same_bits(g2, g3)
    assert same_bits(net.flat_grads, torch.add(torch.add(g1, g2), g3))
    assert same_bits(step.grad_acc, torch.add(g1, g2))
    # every micro-step was a normal training forward: three momentum updates of the running statistics on both networks
    names = [n for n, _ in net.named_buffers()]
    assert names and all(torch.equal(a, b) for a, b in zip(net.buffers(), net_b.buffers()))       # (no nan in a statistic: equal values, equal bits)
    tracked = [b for n, b in net.named_buffers() if n.endswith("num_batches_tracked")]
    assert all(int(b) == 3 for b in tracked)


def test_the_same_batch_twice_under_two_steps_is_one_plain_step_on_it():
    """g + g and the factor 1/2 are exact in binary: parameters, moments, norm and coefficient agree bit for bit with the plain step;
    only the running statistics differ (two momentum updates against one)."""
    kw = dict(clip_grad_norm=1e-3)                                        # (far below the gradient norm of a fresh network: the step is clipped)
    _, net_a, step_a, batches = _setup(accum_steps=2, **kw)
    _, net_b, step_b, _ = _setup(**kw)
    step_a(*batches[0]); step_a(*batches[0])
    step_b(*batches[0])
    torch.cuda.synchronize()
    assert step_a.updated and step_a.step_count == step_b.step_count == 1 and step_b.grad_acc is None
    assert same_bits(net_a.flat_grads, torch.add(net_b.flat_grads, net_b.flat_grads))
    assert same_bits(net_a.flat_params, net_b.flat_params)
    assert same_bits(step_a.exp_avg, step_b.exp_avg) and same_bits(step_a.exp_avg_sq, step_b.exp_avg_sq)
    assert same_bits(step_a._status, step_b._status) and 0 < float(step_a.clip_coef) < 1, "the step was meant to be clipped"
    means = [(a, b) for (n, a), (_, b) in zip(net_a.named_buffers(), net_b.named_buffers()) if n.endswith("running_mean")]
    assert means and any(not same_bits(a, b) for a, b in means)


def test_one_accumulation_step_is_the_default_step_and_allocates_nothing(monkeypatch):
    from structuredetector_amd import _lib as L
    _, net_a, step_a, batches = _setup(accum_steps=1, **OPTIONS)
    _, net_b, step_b, _ = _setup(**OPTIONS)
    assert step_a.grad_acc is None and step_b.grad_acc is None and step_b.accum_steps == 1
    real = L.lib()
    spy = _Spy(real)
    monkeypatch.setattr(L, "_lib", spy)
    for k in range(2):
        la = step_a(*batches[k])
        assert step_a.updated is True and step_a.micro == 0
    monkeypatch.setattr(L, "_lib", real)
    assert "sd_grad_accum" not in spy.calls and step_a.flush() is False
    for k in range(2):
        lb = step_b(*batches[k])
    torch.cuda.synchronize()
    assert same_bits(la, lb) and step_a.step_count == step_b.step_count == 2
    assert same_bits(net_a.flat_params, net_b.flat_params) and same_bits(step_a.ema, step_b.ema)
    assert same_bits(step_a.exp_avg, step_b.exp_avg) and same_bits(step_a.exp_avg_sq, step_b.exp_avg_sq)
    assert same_bits(step_a._status, step_b._status)
    from structuredetector_amd.model.trainer import TrainStep
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError, match="accum_steps"):
            TrainStep(net_b, step_b.args, accum_steps=bad)


def test_flush_ends_a_partial_group_and_does_nothing_at_a_boundary(monkeypatch):
    from structuredetector_amd import _lib as L
    _, net_a, step_a, batches = _setup(accum_steps=4, **OPTIONS)
    _, net_b, step_b, _ = _setup(accum_steps=2, **OPTIONS)
    real = L.lib()
    spy = _Spy(real)
    monkeypatch.setattr(L, "_lib", spy)
    assert step_a.flush() is False                                        # nothing accumulated yet: no launch at all
    assert spy.calls == [] and step_a.step_count == 0 and step_a.updated is False
    monkeypatch.setattr(L, "_lib", real)
    for k in range(2):
        step_a(*batches[k]); step_b(*batches[k])
    assert step_a.micro == 2 and not step_a.updated and step_a.step_count == 0 and step_b.updated and step_b.step_count == 1
    assert step_a.flush() is True
    torch.cuda.synchronize()
    assert step_a.micro == 0 and step_a.updated and step_a.step_count == 1
    assert same_bits(net_a.flat_grads, net_b.flat_grads)
    assert same_bits(net_a.flat_params, net_b.flat_params) and same_bits(step_a.ema, step_b.ema)
    assert same_bits(step_a.exp_avg, step_b.exp_avg) and same_bits(step_a.exp_avg_sq, step_b.exp_avg_sq)
    assert same_bits(step_a._status, step_b._status)
    held = net_a.flat_params.clone()
    spy = _Spy(real)
    monkeypatch.setattr(L, "_lib", spy)
    assert step_a.flush() is False
    monkeypatch.setattr(L, "_lib", real)
    torch.cuda.synchronize()
    assert spy.calls == [] and step_a.step_count == 1 and same_bits(net_a.flat_params, held)


def test_frozen_slots_of_both_buffers_stay_zero_and_the_prefix_is_untouched():
    from structuredetector_amd.model.network import BNParams
    args, net, step, batches = _setup(stages=2, bn=True, accum_steps=2, **OPTIONS)
    off = step.frozen_off
    assert off > 0 and off == net.frozen_range()[1]
    s0 = _state(net, step)
    for k in range(4):                                                    # two groups
        step(*batches[k % 3])
    torch.cuda.synchronize()
    assert step.step_count == 2 and int(step.skipped_steps) == 0
    assert not bool(step.grad_acc[:off].any()) and not bool(net.flat_grads[:off].any())
    assert bool(step.grad_acc[off:].any()) and bool(net.flat_grads[off:].any())
    inside = 0
    for name, mod in net.named_modules():
        if isinstance(mod, BNParams) and name.startswith("down"):          # frozen BatchNorm weight / bias: in the prefix or inside the suffix
            for p in (mod.weight, mod.bias):
                o, n = net._flat_off[id(p)]
                assert not bool(step.grad_acc[o:o + n].any()) and not bool(net.flat_grads[o:o + n].any()), name
                assert same_bits(net.flat_params[o:o + n], s0["p"][o:o + n]), name
                inside += o >= off
    assert inside == 2 * (9 + 13 + 7)                                     # down2 .. down4 (tests/test_gpu_freeze.py)
    assert same_bits(net.flat_params[:off], s0["p"][:off]) and same_bits(step.ema[:off], s0["ema"][:off])
    assert not bool(step.exp_avg[:off].any()) and not bool(step.exp_avg_sq[:off].any())
    assert not same_bits(net.flat_params[off:], s0["p"][off:])


def test_a_nan_in_the_accumulator_skips_the_update():
    args, net, step, batches = _setup(accum_steps=2, clip_grad_norm=0.5)
    s0 = _state(net, step)
    step(*batches[0])
    step.grad_acc[12345] = float("nan")                                   # one micro-gradient was not finite: so is the sum
    step(*batches[1])
    torch.cuda.synchronize()
    assert step.updated is True and step.step_count == 1                  # the optimizer launch ran -- and its guard skipped the update
    assert int(step.skipped_steps) == 1 and float(step.clip_coef) == 0.0 and not np.isfinite(float(step.grad_norm))
    assert _unchanged(net, step, s0)
    assert bool(torch.isnan(net.flat_grads[12345])) and int(torch.isnan(net.flat_grads).sum()) == 1
    # the next group is clean: it overwrites the accumulator and updates
    step(*batches[1]); step(*batches[2])
    torch.cuda.synchronize()
    assert step.step_count == 2 and int(step.skipped_steps) == 1 and float(step.clip_coef) > 0 and not _unchanged(net, step, s0)


# ---- the Trainer --------------------------------------------------------------------------------------------------------------------------
def test_trainer_five_batches_two_per_step_make_three_updates_and_resume_continues(tmp_path, monkeypatch, capsys):
    from structuredetector_amd.model.trainer import Trainer, TrainStep
    from structuredetector_amd.utils.args import Arguments
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    monkeypatch.chdir(tmp_path)
    argv = ["-s", "stem", "--labels", str(tmp_path / "labels.json"), "--synthetic", "10", "--epochs", "1", "-b", "2", "-W", "128", "-H", "128",
            "--accum_steps", "2", "--clip_grad_norm", "0.5"]
    groups, calls = [], []
    inner_update, inner_call = TrainStep._update, TrainStep.__call__

    def update(self, k):
        groups.append(k)
        return inner_update(self, k)

    def call(self, images, targets):
        out = inner_call(self, images, targets)
        calls.append(self.updated)
        return out

    monkeypatch.setattr(TrainStep, "_update", update)
    monkeypatch.setattr(TrainStep, "__call__", call)
    tr = Trainer(Arguments().parse(argv))
    assert tr.step.accum_steps == 2 and tr.batches_per_epoch() == 5 and tr.steps_per_epoch() == 3
    tr.train()
    assert calls == [False, True, False, True, False] and groups == [2, 2, 1]      # the last group is flushed with its one batch
    assert tr.step.step_count == 3 and tr.step.micro == 0 and tr.global_step == 10
    out = capsys.readouterr().out
    assert "gradient accumulation: 2 batches per optimizer step, effective batch 4" in out and "--freeze_bn" in out and "--sync_bn" in out
    assert "(3 steps, 5 batches)" in out
    rows = [json.loads(ln) for ln in (tr.save_dir / "scalars.jsonl").read_text().splitlines()]
    train = [r for r in rows if r["tag"] == "Loss/Train"]
    assert [r["step"] for r in train] == [0, 4, 8] and all(np.isfinite(list(r["values"].values())).all() for r in train)
    assert [r["step"] for r in rows if r["tag"] == "Gradient norm"] == [0, 4, 8]
    # the end-of-epoch checkpoint sits at an update boundary: a resumed run continues from optimizer step 3 with nothing accumulated
    del groups[:], calls[:]
    assert argv[4:8] == ["--synthetic", "10", "--epochs", "1"]
    tr2 = Trainer(Arguments().parse(argv[:4] + ["--synthetic", "10", "--epochs", "2"] + argv[8:] + ["--resume", str(tr.save_dir / "resume.pth")]))
    assert tr2.step.step_count == 3 and tr2.start_epoch == 1 and tr2.step.micro == 0 and tr2.global_step == 10
    assert tr2.step.grad_acc is not None and not bool(tr2.step.grad_acc.any())
    tr2.train()
    assert tr2.step.step_count == 6 and groups == [2, 2, 1] and tr2.global_step == 20
