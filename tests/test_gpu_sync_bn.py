"""Synchronized BatchNorm (`TrainStep(..., sync_bn=True)`, `train --sync_bn`) on the GPU.

  * 2 ranks over gloo (sharing the test GPU, as tests/test_gpu_dp.py) against ONE process that runs the concatenated batch: per-layer
    batch statistics, running statistics, per-rank losses and the summed gradient agree; the same harness with rank-local statistics
    misses the tolerances by >= 10x (the comparison discriminates).  fp32 at 128^2, a 512^2 case whose convs take the epilogue
    statistics paths (checked from the entry points the engine recorded), unequal per-rank batches, and the mixed-precision step;
  * world 1: the split statistics finish is bit-identical to the default step at the production shape (bs = 64, 512^2);
  * 2 ranks over RCCL when two GPUs are visible;
  * `Trainer` end to end with `--sync_bn`: both ranks end with the same BatchNorm buffers; the C-ABI RCCL exchange refuses sync_bn."""
import os
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

TIMEOUT = timedelta(seconds=120)        # a mismatched collective fails instead of hanging
STEPS = 2                               # two steps: the running statistics' momentum and n / (n - 1) on the second update
TOL_FP32 = dict(stats=1e-5, running=1e-5, loss=1e-5, grad=1e-4, grad_total=1e-4)
# 512^2: the default step's own gradients depend on the batch size there.  Measured on the MI355X, one process, no sync_bn: rank 0's
# images twice (B = 4) vs twice the gradient of the images once (B = 2) -- the same mathematics -- differ by up to 1.0e-2 (relative L2)
# on BatchNorm parameters and a few conv weights whose gradients nearly cancel over the pixels (the kernels differ between the two grid
# sizes); the whole gradient measured 2.0e-3 in the two-rank comparison.  Statistics, running statistics and losses keep the fp32 bound.
TOL_FP32_512 = dict(TOL_FP32, grad=3e-2, grad_total=5e-3)
# --amp at 128^2: measured on the MI355X, the two-rank step agrees with the one-process step as closely as fp32 does (largest error
# 2.6e-7 on the statistics, 8.1e-7 on a gradient tensor): the fp32 bounds hold, and the rank-local control misses them by > 10^4
TOL_AMP = TOL_FP32


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port, backend="gloo"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if backend == "nccl":
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, timeout=TIMEOUT, device_id=torch.device("cuda", rank))
    else:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _net(amp, dev=None):
    from structuredetector_amd.model import Network
    from tests.test_host_cpu import make_args
    dev = dev or torch.device("cuda", torch.cuda.current_device())
    args = make_args(2, 1, 20, 40, device=dev, learning_rate=1e-3, use_amp=bool(amp))
    torch.manual_seed(0)
    return args, Network(args, pretrained=False).to(dev).train(), dev


def _data(seed, B, size, args, dev):
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    enc = Encode(args)
    tgt = enc.render(enc.plan(size, size, *synthetic_batch(np.random.default_rng(100 + seed), B, size, size, 2, 1)), dev)
    x = torch.randn(B, 3, size, size, device=dev, generator=torch.Generator(dev).manual_seed(200 + seed))
    return x, tgt


def _tape_stats(tape):
    """(batch mean, invstd) of the 39 BatchNorms of a training forward: stem, (bn1, bn2[, downsample]) per block, the 3 FPN levels."""
    out = [tape["stem"][2:4]]
    for b in tape["blocks"]:
        out += [(b[6], b[7]), (b[10], b[11])] + ([(b[15], b[16])] if b[15] is not None else [])
    out += [(f[7], f[8]) for f in tape["fpn"]]
    assert len(out) == 39
    return [(m.detach().cpu().clone(), i.detach().cpu().clone()) for m, i in out]


def _running(net):
    return [b.detach().cpu().clone() for n, b in net.named_buffers() if n.endswith(("running_mean", "running_var"))]


def _capture_tapes(net):
    tapes = []
    orig = net.forward_train

    def fwd(*a, **k):
        head, tape = orig(*a, **k)
        tapes.append(tape)
        return head, tape
    net.forward_train = fwd
    return tapes


def _dp_worker(rank, world, port, cfg, outdir):
    _init(rank, world, port)
    try:
        from structuredetector_amd.model.trainer import TrainStep
        args, net, dev = _net(cfg["amp"])
        step = TrainStep(net, args, lr=0.0, sync_bn=cfg["sync"])       # lr 0: the weights stay put, the gradients are the step's
        assert step.world == world
        step.sync_parameters()
        net._engine.fuse_bn_bwd = cfg["fuse"]
        if step.bn_sync is not None:
            step.bn_sync.log = []
        x, tgt = _data(rank, cfg["batches"][rank], cfg["size"], args, dev)
        tapes = _capture_tapes(net)
        steps = []
        for _ in range(STEPS):
            loss = step(x, tgt)
            torch.cuda.synchronize()
            steps.append(dict(loss=float(loss[0]), stats=_tape_stats(tapes[-1]), running=_running(net),
                              grads=net.flat_grads.cpu().clone() if rank == 0 else None))
            tapes.clear()
        torch.save(dict(steps=steps, log=list(step.bn_sync.log) if step.bn_sync is not None else []), os.path.join(outdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _reference(cfg):
    """One process, the concatenated batch; dhead = the concatenation of each rank-half's loss gradient."""
    from structuredetector_amd.model.loss import loss_backward, loss_config, loss_forward
    args, net, dev = _net(cfg["amp"])
    net._engine.fuse_bn_bwd = cfg["fuse"]
    data = [_data(r, B, cfg["size"], args, dev) for r, B in enumerate(cfg["batches"])]
    xcat = torch.cat([x for x, _ in data])
    one = torch.ones((), dtype=torch.float32, device=dev)
    steps = []
    for _ in range(STEPS):
        head, tape = net.forward_train(xcat, amp=cfg["amp"])
        dheads, losses, lo = [], [], 0
        for (x, tgt) in data:
            h = head[lo:lo + x.shape[0]].contiguous()
            lo += x.shape[0]
            lcfg = loss_config(args, 2, 1, tgt["anchor_inds"].shape[1], tgt["part_inds"].shape[1])
            desc, keep, out8 = loss_forward(h, tgt, lcfg)
            dheads.append(loss_backward(desc, out8, one, tuple(h.shape)))
            losses.append(float(out8[0]))
        net.backward_from(tape, torch.cat(dheads))
        torch.cuda.synchronize()
        steps.append(dict(losses=losses, stats=_tape_stats(tape), running=_running(net), grads=net.flat_grads.cpu().clone()))
    spans = [net._flat_off[id(p)] for p in net._flat_order]
    return steps, spans


def _run_dp(cfg, tmp_path):
    outdir = tmp_path / ("sync" if cfg["sync"] else "local")
    outdir.mkdir()
    world = len(cfg["batches"])
    mp.spawn(_dp_worker, args=(world, _free_port(), cfg, str(outdir)), nprocs=world, join=True)
    return [torch.load(outdir / f"rank{r}.pt", weights_only=False) for r in range(world)]


def _grad_errors(g, gr, spans):
    return [float((g[o:o + n].double() - gr[o:o + n].double()).norm() / gr[o:o + n].double().norm().clamp_min(1e-30)) for o, n in spans]


def _errors(ranks, ref, spans):
    """Largest error of each kind over both steps: batch mean (scaled by invstd), invstd (relative), running statistics (mean scaled by
    the running std, var relative), per-rank loss (relative), summed gradient per parameter tensor (relative L2)."""
    e = dict(stats=0.0, running=0.0, loss=0.0, grad=0.0, grad_total=0.0)
    for s, rs in enumerate(ref):
        for r, rank in enumerate(ranks):
            mine = rank["steps"][s]
            for (m, i), (mr, ir) in zip(mine["stats"], rs["stats"]):
                e["stats"] = max(e["stats"], float(((m - mr).abs() * ir).max()), float(((i - ir).abs() / ir).max()))
            for k in range(0, len(rs["running"]), 2):
                rm, rv, rmr, rvr = mine["running"][k], mine["running"][k + 1], rs["running"][k], rs["running"][k + 1]
                e["running"] = max(e["running"], float(((rm - rmr).abs() / rvr.sqrt()).max()), float(((rv - rvr).abs() / rvr).max()))
            e["loss"] = max(e["loss"], abs(mine["loss"] - rs["losses"][r]) / max(abs(rs["losses"][r]), 1e-12))
        g, gr = ranks[0]["steps"][s]["grads"].double(), rs["grads"].double()
        e["grad_total"] = max(e["grad_total"], float((g - gr).norm() / gr.norm()))
        for t, rel in enumerate(_grad_errors(g, gr, spans)):
            if rel > e["grad"]:
                e["grad"], e["grad_worst"] = rel, (s, t)
    return e


def _check(cfg, tmp_path, tol, control=True, control_factor=10.0):
    ref, spans = _reference(cfg)
    ranks = _run_dp(cfg, tmp_path)
    err = _errors(ranks, ref, spans)
    print("sync_bn errors", cfg, err)
    for k, t in tol.items():
        assert err[k] <= t, (k, err[k], t, err)
    for s in range(STEPS):                     # running statistics: the same bits on every rank
        for r in range(1, len(ranks)):
            assert all(torch.equal(a, b) for a, b in zip(ranks[0]["steps"][s]["running"], ranks[r]["steps"][s]["running"]))
    if control:
        local = _run_dp(dict(cfg, sync=False), tmp_path)
        bad = _errors(local, ref, spans)
        print("rank-local errors", cfg, bad)
        for k in ("stats", "grad"):
            assert bad[k] >= control_factor * tol[k], (k, bad[k], tol[k], bad)
    return ranks


def test_two_ranks_fp32_equal_one_process_on_the_concatenated_batch(tmp_path):
    cfg = dict(sync=True, amp=False, fuse=False, batches=(2, 2), size=128)
    ranks = _check(cfg, tmp_path, TOL_FP32)
    log = ranks[0]["log"]
    assert len(log) == STEPS * 2 * 39 and log == ranks[1]["log"]          # every BatchNorm, both directions, same order on both ranks


def test_two_ranks_fp32_epilogue_statistics_paths(tmp_path):
    """512^2: the conv epilogues produce the partial statistics (sd_conv2d_fwd_bn_stats' fused form, and with fuse_bn_bwd the
    data-gradient epilogue's BatchNorm-backward reduction), not only the two-pass fallback."""
    cfg = dict(sync=True, amp=False, fuse=True, batches=(2, 2), size=512)
    ranks = _check(cfg, tmp_path, TOL_FP32_512, control=False)
    log = ranks[0]["log"]
    assert "sd_conv2d_fwd_bn_sums" in log and "sd_conv2d_fwd_bn_sums:two-pass" in log
    assert "sd_conv2d_dgrad_bn_reduce_sums" in log and "sd_conv2d_stem_fwd_bn_sums" in log and "sd_maxpool_bn_relu_bwd_reduce" in log


def test_unequal_rank_batches_use_the_global_count(tmp_path):
    cfg = dict(sync=True, amp=False, fuse=False, batches=(1, 3), size=128)
    _check(cfg, tmp_path, TOL_FP32, control=False)


def test_two_ranks_mixed_precision(tmp_path):
    cfg = dict(sync=True, amp=True, fuse=False, batches=(2, 2), size=128)
    ranks = _check(cfg, tmp_path, TOL_AMP)
    log = ranks[0]["log"]
    assert any(n.startswith("sd_conv2d_fwd_bf16_bn_sums") for n in log) and "sd_bn_bwd_reduce_bf16" in log


def _world1_run(amp, fuse, sync):
    from structuredetector_amd.model.trainer import TrainStep
    args, net, dev = _net(amp)
    net._engine.fuse_bn_bwd = fuse
    step = TrainStep(net, args, sync_bn=sync)
    assert step.world == 1
    if sync:
        step.bn_sync.log = []
    x, tgt = _data(7, 64, 512, args, dev)
    losses = [step(x, tgt).cpu().clone() for _ in range(STEPS)]
    torch.cuda.synchronize()
    out = dict(losses=losses, params=net.flat_params.cpu().clone(), grads=net.flat_grads.cpu().clone(),
               buffers=[b.cpu().clone() for b in net.buffers()], log=list(step.bn_sync.log) if sync else None)
    del net, step
    torch.cuda.empty_cache()
    return out


def _max_diffs(a, b):
    cat = lambda r: torch.cat([t.double().flatten() for t in r["losses"] + [r["params"], r["grads"]] + r["buffers"]])
    return float((cat(a) - cat(b)).abs().max())


@pytest.mark.parametrize("amp,fuse", [(False, False), (False, True), (True, False)], ids=["fp32", "fp32-fused-bn-bwd", "amp"])
def test_world1_split_finish_is_bit_identical(amp, fuse):
    """sync_bn=True with one rank runs the split statistics finish (phase 1 -> fp64 sums -> phase 2) without a collective: parameters,
    gradients, BatchNorm buffers and losses equal the default step's bit for bit, two steps at bs = 64, 512^2.
    --amp: the DEFAULT mixed-precision step at this shape is not bit-reproducible from run to run (measured on the MI355X: two default
    runs from the same state already differ in the first loss), so there the split step must stay within that run-to-run spread."""
    a = _world1_run(amp, fuse, False)
    b = _world1_run(amp, fuse, True)
    if amp:
        spread = _max_diffs(a, _world1_run(amp, fuse, False))
        assert _max_diffs(a, b) <= 4.0 * spread, (_max_diffs(a, b), spread)
    else:
        assert all(torch.equal(x, y) for x, y in zip(a["losses"], b["losses"]))
        assert torch.equal(a["params"], b["params"]) and torch.equal(a["grads"], b["grads"])
        assert all(torch.equal(x, y) for x, y in zip(a["buffers"], b["buffers"]))
    log = b["log"]
    assert len(log) == STEPS * 2 * 39
    fwd = "sd_conv2d_fwd_bf16_bn_sums" if amp else "sd_conv2d_fwd_bn_sums"
    assert fwd in log                                                   # the fused epilogue statistics at the production shape
    if fuse:
        assert "sd_conv2d_dgrad_bn_reduce_sums" in log


def _rccl_worker(rank, world, port, outdir):
    _init(rank, world, port, backend="nccl")
    try:
        from structuredetector_amd.model.trainer import TrainStep
        args, net, dev = _net(False, torch.device("cuda", rank))
        step = TrainStep(net, args, sync_bn=True)
        step.sync_parameters()
        x, tgt = _data(rank, 2, 128, args, dev)
        for _ in range(STEPS):
            step(x, tgt)
        torch.cuda.synchronize()
        torch.save(dict(buffers=[b.cpu() for b in net.buffers()], params=net.flat_params.cpu()), os.path.join(outdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs (RCCL places one rank per device)")
def test_two_rank_sync_bn_over_rccl_when_two_gpus_are_present(tmp_path):
    mp.spawn(_rccl_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(2))
    assert all(torch.equal(a, b) for a, b in zip(r0["buffers"], r1["buffers"]))
    assert torch.equal(r0["params"], r1["params"])


def _trainer_worker(rank, world, port, tmp, outdir):
    _init(rank, world, port)
    try:
        import json
        from pathlib import Path

        from structuredetector_amd import _lib as L
        from structuredetector_amd.model.trainer import Trainer, TrainStep
        from structuredetector_amd.utils.args import Arguments
        tmp = Path(tmp)
        os.chdir(tmp)
        (tmp / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
        argv = ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp / "labels.json"), "-b", "2", "-e", "1",
                "--synthetic", "8", "--steps", "2", "--sync_bn"]
        args = Arguments().parse(argv)
        assert args.sync_bn is True
        torch.manual_seed(5)
        tr = Trainer(args)
        assert tr.step.world == world and tr.step.sync_bn and tr.step.bn_sync is not None
        import contextlib
        import io
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            tr.train()
        torch.cuda.synchronize()
        refused = ""
        try:
            TrainStep(tr.net, args, exchange="rccl", sync_bn=True)
        except L.SdError as e:
            refused = str(e)
        torch.save(dict(buffers=[b.cpu() for b in tr.net.buffers()], step_count=tr.step.step_count, refused=refused, printed=printed.getvalue()),
                   os.path.join(outdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_trainer_end_to_end_with_sync_bn(tmp_path):
    outdir = tmp_path / "out"
    outdir.mkdir()
    mp.spawn(_trainer_worker, args=(2, _free_port(), str(tmp_path), str(outdir)), nprocs=2, join=True)
    r0, r1 = (torch.load(outdir / f"rank{r}.pt", weights_only=False) for r in range(2))
    assert r0["step_count"] == r1["step_count"] == 2
    assert all(torch.equal(a, b) for a, b in zip(r0["buffers"], r1["buffers"]))       # images differ per rank: only sync_bn makes these agree
    assert any(not torch.equal(b, torch.zeros_like(b)) for b in r0["buffers"][:1])    # the running mean moved
    assert "sync_bn" in r0["refused"] and "process group" in r0["refused"]
    assert "synchronized BatchNorm: on" in r0["printed"]
