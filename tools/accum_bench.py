#!/usr/bin/env python3
"""Gradient accumulation (`train --accum_steps K`, `sd_grad_accum`) measured on the production flat buffer (the ResNet-34 + FPN-128 network:
21.85 M floats) and on the production step (batch 64, 512x512, fp32 and --amp), in two parts:

  kernels   `sd_grad_accum` over the whole buffer in both modes, over the five bucket ranges as the step launches them (one launch per
            parameter group, timed as the group of five), and a device-to-device copy of the same buffer, all in one process, alternating:
            one pair of stream events per launch (per group of five), `--launches` timed after `--warmup` of each.  Bytes per second from the
            bytes each moves: add 12 per float (two reads, one write), overwrite and copy 8.
  steps     `TrainStep(accum_steps=4)`: one pair of stream events per call, the calls sorted by `updated` into micro-steps and updating
            steps; beside it this tree's plain step.  With --parent DIR (a built checkout of the parent commit) the parent's plain step and
            its optimizer launch alone (`sd_adam_step` over the same buffer) are measured in alternating child processes, `--rounds` each.

  accum_bench.py [--out profiles/accum_bench.json] [--launches 100] [--warmup 10] [--steps 24] [--step-warmup 8] [--parent DIR] [--rounds 2] [--no-steps]
  accum_bench.py --measure TREE --amp 0|1 --accum K      (the child: prints one JSON line; TREE's package is the one imported; K = 0: the plain
        step of a tree that may not know `accum_steps`, and its optimizer launch)"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
BATCH, SIDE, ACCUM = 64, 512, 4
STAGES = ("fpn_head", "down4", "down3", "down2", "down1_stem")          # TrainStep.STAGES: the order of the step's five launches


def summary(us):
    us = sorted(us)
    q = statistics.quantiles(us, n=4)
    return dict(median=round(statistics.median(us), 2), min=round(us[0], 2), max=round(us[-1], 2), q1=round(q[0], 2), q3=round(q[2], 2), launches=len(us))


def kernels(launches, warmup):
    sys.path.insert(0, str(HERE))
    import torch
    from bench import make_args
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model import Network
    lib, dev = L.lib(), torch.device("cuda")
    net = Network(make_args(dev), pretrained=False).to(dev)
    n, ranges = net.flat_params.numel(), net.stage_ranges()
    del net
    gen = torch.Generator(dev).manual_seed(0)
    acc, grad = torch.randn(n, device=dev, generator=gen) * 1e-3, torch.randn(n, device=dev, generator=gen) * 1e-3

    def accum(lo, hi, overwrite):
        L.check(lib.sd_grad_accum(acc.data_ptr() + 4 * lo, grad.data_ptr() + 4 * lo, hi - lo, overwrite, L.stream()), "sd_grad_accum")

    def buckets():
        for name in STAGES:
            accum(*ranges[name], 0)

    # (the sums stay finite: 1e-3-sized values, a few hundred additions)
    cases = {"add": (lambda: accum(0, n, 0), 12 * n), "overwrite": (lambda: accum(0, n, 1), 8 * n), "add_five_buckets": (buckets, 12 * n),
             "copy_d2d": (lambda: acc.copy_(grad), 8 * n)}
    times = {name: [] for name in cases}
    for k in range(warmup + launches):
        for name, (run, _) in cases.items():                # alternating: no case always runs behind the same other one
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if k >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert bool(torch.isfinite(acc).all())
    out = {}
    for name, us in times.items():
        moved = cases[name][1]
        s = summary(us)
        out[name] = dict(s, bytes_moved=moved, GBps_at_median=round(moved / s["median"] / 1e3, 1), GBps_at_slowest=round(moved / s["max"] / 1e3, 1),
                         GBps_at_fastest=round(moved / s["min"] / 1e3, 1))
    return dict(n=n, bucket_floats={name: ranges[name][1] - ranges[name][0] for name in STAGES}, us=out,
                note="both buffers together are 175 MB: they fit the 256 MB last-level cache, so rates above the HBM peak are cache hits")


def measure(tree, amp, accum, steps, warmup):
    sys.path.insert(0, str(tree))
    import numpy as np
    import torch
    from bench import make_args
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    dev = torch.device("cuda")
    args = make_args(dev)
    args.use_amp = bool(amp)
    enc = Encode(args)
    x = torch.randn(BATCH, 3, SIDE, SIDE, device=dev, generator=torch.Generator(dev).manual_seed(0))
    plan = enc.upload(enc.plan(SIDE, SIDE, *synthetic_batch(np.random.default_rng(0), BATCH, SIDE, SIDE, 2, 1)))
    torch.manual_seed(0)
    net = Network(args, pretrained=False).to(dev).train()
    step = TrainStep(net, args, accum_steps=accum) if accum else TrainStep(net, args)
    for _ in range(warmup):
        step(x, enc.render_device(plan))
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    updated = []
    torch.cuda.synchronize()
    marks[0].record()
    for k in range(steps):
        loss = step(x, enc.render_device(plan))
        marks[k + 1].record()
        updated.append(bool(getattr(step, "updated", True)))
    torch.cuda.synchronize()
    ms = [marks[k].elapsed_time(marks[k + 1]) for k in range(steps)]
    out = dict(amp=bool(amp), accum_steps=accum or 1, loss=float(loss[0]))

    def put(key, values):
        values = sorted(values)
        out[key] = dict(median=round(statistics.median(values), 3), min=round(values[0], 3), max=round(values[-1], 3), calls=len(values))

    if accum > 1:
        put("micro_step_ms", [t for t, u in zip(ms, updated) if not u])
        put("updating_step_ms", [t for t, u in zip(ms, updated) if u])
    else:
        put("step_ms", ms)
        # the optimizer launch of the plain step alone, on the step's own buffers (gradient zeroed: the weights do not move)
        lib, n = L.lib(), net.flat_params.numel()
        net.flat_grads.zero_()
        us = []
        for k in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.check(lib.sd_adam_step(net.flat_params.data_ptr(), net.flat_grads.data_ptr(), step.exp_avg.data_ptr(), step.exp_avg_sq.data_ptr(), n,
                                     step.step_count + 1 + k, 1e-3, 0.9, 0.999, 1e-8, 1.0, L.stream()), "sd_adam_step")
            e1.record()
            e1.synchronize()
            if k >= 5:
                us.append(e0.elapsed_time(e1))
        put("adam_launch_ms", us)
    print(json.dumps(out))


def child(tree, amp, accum, steps, warmup):
    """a fresh process per measurement (its own allocator, its own warm-up); the last line of its output is the JSON"""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--measure", str(tree), "--amp", str(int(amp)), "--accum", str(accum), "--steps", str(steps),
           "--step-warmup", str(warmup)]
    done = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return json.loads(done.stdout.strip().splitlines()[-1])


def steps_report(parent, rounds, steps, warmup, accum_us):
    rows = []
    for amp in (0, 1):
        runs = {"parent": [], "this_plain": [], "this_accum": []}
        for _ in range(rounds):                             # alternating: no tree always runs behind the other
            if parent:
                runs["parent"].append(child(Path(parent).resolve(), amp, 0, steps, warmup))
            runs["this_plain"].append(child(HERE, amp, 1, steps, warmup))
            runs["this_accum"].append(child(HERE, amp, ACCUM, steps, warmup))
        row = dict(amp=bool(amp), runs=runs)
        med = lambda key, field: [r[field]["median"] for r in runs[key]]
        row["this_plain_step_ms"] = med("this_plain", "step_ms")
        row["micro_step_ms"], row["updating_step_ms"] = med("this_accum", "micro_step_ms"), med("this_accum", "updating_step_ms")
        if parent:
            p, adam = med("parent", "step_ms"), med("parent", "adam_launch_ms")
            row.update(parent_step_ms=p, parent_adam_launch_ms=adam, parent_spread_ms=round(max(p) - min(p), 3))
            # the bound of the feature: a micro-step is the parent's step without its optimizer launch, plus the accumulate launches
            bound = statistics.median(p) - statistics.median(adam) + accum_us / 1e3 + (max(p) - min(p))
            row.update(micro_step_bound_ms=round(bound, 3), micro_step_within_bound=bool(statistics.median(row["micro_step_ms"]) <= bound))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(HERE / "profiles" / "accum_bench.json"))
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--step-warmup", type=int, default=8)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--measure", default=None)
    ap.add_argument("--amp", type=int, default=0)
    ap.add_argument("--accum", type=int, default=ACCUM)
    a = ap.parse_args()
    if a.measure:
        return measure(Path(a.measure), a.amp, a.accum, a.steps, a.step_warmup)
    if a.launches < 50 or a.steps < 20 or a.steps % ACCUM or a.step_warmup % ACCUM:
        ap.error(f"--launches >= 50, --steps >= 20; --steps and --step-warmup multiples of {ACCUM} (whole accumulation groups)")
    report = dict(timing=f"kernels: one pair of stream events per launch, the cases alternating, {a.launches} timed after {a.warmup}; microseconds",
                  kernels=kernels(a.launches, a.warmup))
    if not a.no_steps:
        accum_us = report["kernels"]["us"]["add_five_buckets"]["median"]
        report["steps"] = dict(workload=f"TrainStep, batch {BATCH}, {SIDE}x{SIDE}, synthetic targets, plain Adam, accum_steps {ACCUM}, one GPU",
                               timing=f"one pair of stream events per call after {a.step_warmup} warm-up calls, {a.steps} calls; a child process per "
                               f"measurement, the trees alternating, {a.rounds} round(s); milliseconds; bound = parent step - parent optimizer "
                               "launch + the five accumulate launches + the parent's spread between rounds",
                               rows=steps_report(a.parent, a.rounds, a.steps, a.step_warmup, accum_us))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(report, indent=1) + "\n")
    for name, r in report["kernels"]["us"].items():
        print(f"{name}: median {r['median']} us [{r['min']}, {r['max']}] {r['GBps_at_median']} GB/s [{r['GBps_at_slowest']}, {r['GBps_at_fastest']}]")
    for r in report.get("steps", {}).get("rows", []):
        print({k: v for k, v in r.items() if k != "runs"})


if __name__ == "__main__":
    main()
