"""Gradient accumulation under data parallelism, as tests/test_gpu_optim_dp.py runs the optimizer options: two processes share the one
GPU of the test box and exchange gradients through gloo.  With `accum_steps` = 2 the gradients travel once per optimizer step: the
first micro-step starts no gradient all-reduce, the second one per bucket of the plan, each over the accumulated total; every rank then
holds the same sum and takes the same clipped step, which equals one single-process step on the mean of the four gradients."""
import os
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_gpu_dp import _free_port, _setup
from tests.test_gpu_network import close

pytestmark = pytest.mark.gpu
MAX_NORM = 1e-3                              # (a norm far below any gradient of a freshly initialised network: the step is clipped)
CHILD_SECONDS = 240
ADAM_TOL = 1e-6                              # tests/test_gpu_network.py: sd_adam_step against torch.optim.Adam
ACCUM = 2


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from structuredetector_amd.model.trainer import TrainStep
        args, net, x0, t0 = _setup(ACCUM * rank)                     # this rank's two batches: seeds 2 r and 2 r + 1
        _, _, x1, t1 = _setup(ACCUM * rank + 1)
        step = TrainStep(net, args, clip_grad_norm=MAX_NORM, accum_steps=ACCUM)
        assert step.world == 2
        step.sync_parameters()
        # every all-reduce whose tensor lies inside the flat gradient buffer, with the micro-step it was started in
        seen, phase = [], [0]
        inner = dist.all_reduce
        base, size = net.flat_grads.data_ptr(), 4 * net.flat_grads.numel()

        def counting(tensor, *a, **kw):
            if base <= tensor.data_ptr() < base + size:
                seen.append((phase[0], (tensor.data_ptr() - base) // 4, tensor.numel()))
            return inner(tensor, *a, **kw)

        dist.all_reduce = counting
        try:
            phase[0] = 1
            step(x0, t0)
            torch.cuda.synchronize()
            first = (step.updated, step.step_count, step.micro)
            phase[0] = 2
            step(x1, t1)
            torch.cuda.synchronize()
        finally:
            dist.all_reduce = inner
        plan = sorted(step._groups().values())
        out[rank] = (net.flat_params.cpu(), step.grad_norm.cpu(), step.clip_coef.cpu(), int(step.skipped_steps), net.flat_grads.cpu(), seen, plan,
                     first, (step.updated, step.step_count, step.micro))
    finally:
        dist.destroy_process_group()


def test_two_ranks_exchange_once_per_update_stay_identical_and_match_the_mean_gradient_step():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model.loss import loss_backward, loss_config, loss_forward
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    ctx = mp.spawn(_worker, args=(world, port, out), nprocs=world, join=False)
    deadline = time.monotonic() + CHILD_SECONDS
    while not ctx.join(timeout=5):               # (raises if a rank failed)
        if time.monotonic() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail(f"a rank did not finish its two micro-steps within {CHILD_SECONDS} s")
    (p0, norm0, coef0, skipped0, sum0, seen0, plan0, first0, last0), (p1, norm1, coef1, skipped1, sum1, seen1, plan1, first1, last1) = out[0], out[1]
    # gradient all-reduces: none in the first micro-step, one per bucket of the plan in the second
    for seen, plan, first, last in ((seen0, plan0, first0, last0), (seen1, plan1, first1, last1)):
        assert first == (False, 0, 1) and last == (True, 1, 0)
        assert len(plan) == 5 and [ph for ph, _, _ in seen] == [2] * 5, seen
        assert sorted((lo, lo + n) for _, lo, n in seen) == plan
    assert torch.equal(p0, p1), "ranks diverged"
    assert torch.equal(sum0, sum1)                                   # the exchanged total: the same sum on both ranks
    assert torch.equal(norm0, norm1) and torch.equal(coef0, coef1) and skipped0 == skipped1 == 0
    assert 0 < float(coef0) < 1, "the step was meant to be clipped"
    # reference: the four gradients computed alone, their mean, one clipped step on the initial weights
    grads = []
    for s in range(ACCUM * world):
        args, net, x, tgt = _setup(s)
        head, tape = net.forward_train(x)
        cfg = loss_config(args, 2, 1, 20, 40)
        desc, keep, out8 = loss_forward(head, tgt, cfg)
        dhead = loss_backward(desc, out8, torch.ones((), device=head.device), tuple(head.shape))
        net.backward_from(tape, dhead)
        grads.append(net.flat_grads.clone())
        if s == 0:
            init = net.flat_params.clone()
    mean_g = (((grads[0] + grads[1]) + (grads[2] + grads[3])) * 0.25).contiguous()
    close(sum0 * 0.25, mean_g.cpu(), ADAM_TOL)
    n = init.numel()
    m = torch.zeros_like(init); v = torch.zeros_like(init)
    lib = L.lib()
    partials = torch.empty(lib.sd_grad_sumsq_workspace_bytes(n) // 8, dtype=torch.float64, device=init.device)
    status = torch.zeros(4, dtype=torch.int32, device=init.device)
    L.check(lib.sd_grad_sumsq(mean_g.data_ptr(), n, partials.data_ptr(), partials.numel() * 8, L.stream()))
    L.check(lib.sd_optim_step(init.data_ptr(), mean_g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.0,
                              None, MAX_NORM, partials.data_ptr(), partials.numel(), None, 0.0, status.data_ptr(), L.stream()))
    torch.cuda.synchronize()
    close(p0, init.cpu(), ADAM_TOL)
    want_norm = float(mean_g.double().norm())
    assert abs(float(norm0) - want_norm) <= 1e-6 * want_norm
    assert abs(float(status.view(torch.float32)[0]) - want_norm) <= 1e-6 * want_norm
