"""The optimizer options under data parallelism, as tests/test_gpu_dp.py runs the plain step: two processes share the one GPU of the
test box and exchange gradients through gloo.  Nothing new is exchanged: every rank computes the global norm from the same reduced
gradient buffer, so the clipped, decayed update keeps the ranks bit-identical; it equals one single-process step on the mean gradient."""
import os
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_gpu_dp import _free_port, _setup
from tests.test_gpu_network import close

pytestmark = pytest.mark.gpu
WEIGHT_DECAY, MAX_NORM = 0.05, 1e-3          # (a norm far below any gradient of a freshly initialised network: the step is clipped)
CHILD_SECONDS = 240
ADAM_TOL = 1e-6                              # tests/test_gpu_network.py: sd_adam_step against torch.optim.Adam


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from structuredetector_amd.model.trainer import TrainStep
        args, net, x, tgt = _setup(rank)
        step = TrainStep(net, args, weight_decay=WEIGHT_DECAY, clip_grad_norm=MAX_NORM)
        assert step.world == 2
        step.sync_parameters()
        step(x, tgt)
        torch.cuda.synchronize()
        out[rank] = (net.flat_params.cpu(), step.grad_norm.cpu(), step.clip_coef.cpu(), int(step.skipped_steps))
    finally:
        dist.destroy_process_group()


def test_two_rank_clipped_decayed_step_keeps_ranks_identical_and_matches_the_mean_gradient_step():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model.loss import loss_backward, loss_config, loss_forward
    from structuredetector_amd.model.trainer import TrainStep
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    ctx = mp.spawn(_worker, args=(world, port, out), nprocs=world, join=False)
    deadline = time.monotonic() + CHILD_SECONDS
    while not ctx.join(timeout=5):               # (raises if a rank failed)
        if time.monotonic() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail(f"a rank did not finish its one step within {CHILD_SECONDS} s")
    (p0, norm0, coef0, skipped0), (p1, norm1, coef1, skipped1) = out[0], out[1]
    assert torch.equal(p0, p1), "ranks diverged"
    assert torch.equal(norm0, norm1) and torch.equal(coef0, coef1) and skipped0 == skipped1 == 0
    assert 0 < float(coef0) < 1, "the step was meant to be clipped"
    # reference: each rank's gradient computed alone, their mean, one clipped and decayed step on rank 0's initial weights
    grads = []
    for r in range(world):
        args, net, x, tgt = _setup(r)
        head, tape = net.forward_train(x)
        cfg = loss_config(args, 2, 1, 20, 40)
        desc, keep, out8 = loss_forward(head, tgt, cfg)
        dhead = loss_backward(desc, out8, torch.ones((), device=head.device), tuple(head.shape))
        net.backward_from(tape, dhead)
        grads.append(net.flat_grads.clone())
        if r == 0:
            init = net.flat_params.clone()
            mask = TrainStep.build_decay_mask(net)
    mean_g = ((grads[0] + grads[1]) * 0.5).contiguous()
    n = init.numel()
    m = torch.zeros_like(init); v = torch.zeros_like(init)
    lib = L.lib()
    partials = torch.empty(lib.sd_grad_sumsq_workspace_bytes(n) // 8, dtype=torch.float64, device=init.device)
    status = torch.zeros(4, dtype=torch.int32, device=init.device)
    L.check(lib.sd_grad_sumsq(mean_g.data_ptr(), n, partials.data_ptr(), partials.numel() * 8, L.stream()))
    L.check(lib.sd_optim_step(init.data_ptr(), mean_g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, WEIGHT_DECAY,
                              mask.data_ptr(), MAX_NORM, partials.data_ptr(), partials.numel(), None, 0.0, status.data_ptr(), L.stream()))
    torch.cuda.synchronize()
    close(p0, init.cpu(), ADAM_TOL)
    want_norm = float(mean_g.double().norm())
    assert abs(float(norm0) - want_norm) <= 1e-6 * want_norm
    assert abs(float(status.view(torch.float32)[0]) - want_norm) <= 1e-6 * want_norm
