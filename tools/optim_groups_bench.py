#!/usr/bin/env python3
"""The grouped optimizer launch against the masked one, on the production flat buffer (the ResNet-34 + FPN-128 network: 21.85 M floats), decay +
clipping + EMA on, in one process:

  sd_optim_step          with the decay mask of `TrainStep.build_decay_mask`
  sd_optim_groups_step   with the 14 groups of `Network.optim_groups()` (the multipliers of --backbone_lr_mult 0.1 --lr_layer_decay 0.5)

Both read the same partials of one `sd_grad_sumsq` call; only the update launch is timed: one pair of stream events per launch, the two entry
points alternating, `--launches` timed launches each after `--warmup` of each.  Then the whole `TrainStep` (batch 64, 512x512, fp32 and --amp)
with and without `lr_mults`, one pair of events per step.

  optim_groups_bench.py [--out profiles/optim_groups_bench.json] [--launches 100] [--warmup 10] [--steps 20] [--step-warmup 5] [--no-steps]"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(HERE))
BATCH, SIDE = 64, 512
LR, B1, B2, EPS, WD, MAX_NORM, EMA_DECAY = 1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, 0.999
MULT, LAYER_DECAY = 0.1, 0.5


def summary(us):
    us = sorted(us)
    q = statistics.quantiles(us, n=4)
    return dict(median=round(statistics.median(us), 2), min=round(us[0], 2), max=round(us[-1], 2), q1=round(q[0], 2), q3=round(q[2], 2), launches=len(us))


def kernels(torch, args, launches, warmup):
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    from structuredetector_amd.utils.args import stage_lr_mults
    lib, dev = L.lib(), args.device
    net = Network(args, pretrained=False).to(dev)
    n = net.flat_params.numel()
    mask = TrainStep.build_decay_mask(net)
    ids, groups = net.optim_groups()
    ids = ids.to(dev)
    mults = stage_lr_mults(MULT, LAYER_DECAY)
    lr_mul = (C.c_float * len(groups))(*(mults[stage] for stage, _ in groups))
    wd_mul = (C.c_float * len(groups))(*(float(decayed) for _, decayed in groups))
    gen = torch.Generator(dev).manual_seed(0)
    grad = torch.randn(n, device=dev, generator=gen) * 1e-3
    partials = torch.empty(lib.sd_grad_sumsq_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
    L.check(lib.sd_grad_sumsq(grad.data_ptr(), n, partials.data_ptr(), partials.numel() * 8, L.stream()), "sd_grad_sumsq")
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    # a set of buffers per entry point: neither finds the other's lines in the caches, both walk the same number of bytes
    state = {name: [net.flat_params.detach().clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), net.flat_params.detach().clone()]
             for name in ("sd_optim_step", "sd_optim_groups_step")}
    del net

    def launch(name, step):
        p, m, v, ema = state[name]
        head = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, LR, B1, B2, EPS, 1.0, WD)
        tail = (MAX_NORM, partials.data_ptr(), partials.numel(), ema.data_ptr(), EMA_DECAY, status.data_ptr(), L.stream())
        if name == "sd_optim_step":
            L.check(lib.sd_optim_step(*head, mask.data_ptr(), *tail), name)
        else:
            L.check(lib.sd_optim_groups_step(*head, ids.data_ptr(), lr_mul, wd_mul, len(groups), *tail), name)

    times = {name: [] for name in state}
    for k in range(warmup + launches):
        for name in state:                                  # alternating: neither always runs behind the other
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(name, k + 1)
            e1.record()
            e1.synchronize()
            if k >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert int(status[2]) == 0, "a launch was skipped: the norm was not finite"
    moved = n * 4 * 9 + n // 4                              # p, m, v, ema read and written, grad read, one byte per 16 bytes of parameters
    out = {name: dict(summary(us), GBps_at_median=round(moved / statistics.median(us) / 1e3, 1)) for name, us in times.items()}
    return dict(n=n, groups=len(groups), bytes_moved=moved, options=dict(weight_decay=WD, clip_grad_norm=MAX_NORM, ema_decay=EMA_DECAY), us=out)


def steps(torch, args, count, warmup):
    import numpy as np
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    from structuredetector_amd.utils.args import stage_lr_mults
    dev = args.device
    x = torch.randn(BATCH, 3, SIDE, SIDE, device=dev, generator=torch.Generator(dev).manual_seed(0))
    out = []
    for amp in (False, True):
        args.use_amp = amp
        enc = Encode(args)
        plan = enc.upload(enc.plan(SIDE, SIDE, *synthetic_batch(np.random.default_rng(0), BATCH, SIDE, SIDE, 2, 1)))
        for mults in (None, stage_lr_mults(MULT, 1.0)):
            torch.manual_seed(0)
            net = Network(args, pretrained=False).to(dev).train()
            step = TrainStep(net, args, lr_mults=mults)
            for _ in range(warmup):
                step(x, enc.render_device(plan))
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
            torch.cuda.synchronize()
            marks[0].record()
            for k in range(count):
                step(x, enc.render_device(plan))
                marks[k + 1].record()
            torch.cuda.synchronize()
            ms = sorted(marks[k].elapsed_time(marks[k + 1]) for k in range(count))
            out.append(dict(amp=amp, backbone_lr_mult=None if mults is None else MULT, steps=count, step_ms_median=round(statistics.median(ms), 3),
                            step_ms_min=round(ms[0], 3), step_ms_max=round(ms[-1], 3)))
            del net, step
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(HERE / "profiles" / "optim_groups_bench.json"))
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true")
    a = ap.parse_args()
    if a.launches < 50:
        ap.error("--launches: the median is taken over at least 50 launches of each entry point")
    import torch
    from bench import make_args
    args = make_args(torch.device("cuda"))
    report = dict(timing=f"one pair of stream events per launch, the two entry points alternating, {a.launches} timed launches each after "
                  f"{a.warmup}; microseconds", kernels=kernels(torch, args, a.launches, a.warmup))
    if not a.no_steps:
        report["steps"] = dict(workload=f"TrainStep, batch {BATCH}, {SIDE}x{SIDE}, synthetic targets, plain Adam; lr_mults = --backbone_lr_mult {MULT}",
                               timing=f"one pair of stream events per step after {a.step_warmup} warm-up steps", table=steps(torch, args, a.steps, a.step_warmup))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(report, indent=1) + "\n")
    for name, r in report["kernels"]["us"].items():
        print(f"{name}: median {r['median']} us [{r['min']}, {r['max']}] {r['GBps_at_median']} GB/s")
    for r in report.get("steps", {}).get("table", []):
        print(f"{'amp ' if r['amp'] else 'fp32'} backbone_lr_mult {r['backbone_lr_mult']}: {r['step_ms_median']} ms [{r['step_ms_min']}, {r['step_ms_max']}]")


if __name__ == "__main__":
    main()
