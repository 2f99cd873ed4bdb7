#!/usr/bin/env python3
"""Step time of `TrainStep` with frozen trunk stages (`Network.freeze`, `train --freeze_stages N [--freeze_bn]`): bs = 64, 512x512, fp32 and
`--amp`, N in {0, 1, 2, 3, 5}, with and without frozen BatchNorm.  Per configuration: a fresh network and step, warm-up steps, then one pair
of stream events around every timed step; the median and the quartiles of those are reported.

  freeze_bench.py [--out profiles/freeze_bench.json] [--steps 20] [--warmup 5] [--parent DIR] [--rounds 2]
        every configuration in one child process per precision.  --parent DIR: a built checkout of the parent commit; its default step and this
        tree's N = 0 step are then measured in alternating child processes (`--rounds` each) and both medians and the spread between rounds
        are written beside the table.
  freeze_bench.py --measure TREE --amp 0|1 --configs 0:0,2:1,...      (the child: prints one JSON line; TREE's package is the one imported)
  freeze_bench.py --kernels        the frozen-BatchNorm backward and sd_bn_bwd_apply on M = 64 * 128 * 128, C = 64, fp32 and bf16, ten calls each,
        and three steps with --freeze_stages 2 --freeze_bn: the workload of a `rocprofv3 --kernel-trace --stats` run
        (--kernels-stages N / --kernels-bn 0|1 choose the step).
  freeze_bench.py --kernel-table TRACE.csv      that run's *_kernel_trace.csv -> median kernel times and bytes moved, per precision and place"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
CONFIGS = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (5, 0), (5, 1)]
BATCH, SIDE = 64, 512


def setup(tree, amp):
    sys.path.insert(0, str(tree))
    import numpy as np
    import torch
    from bench import make_args
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    dev = torch.device("cuda")
    args = make_args(dev)
    args.use_amp = bool(amp)
    enc = Encode(args)
    x = torch.randn(BATCH, 3, SIDE, SIDE, device=dev, generator=torch.Generator(dev).manual_seed(0))
    plan = enc.upload(enc.plan(SIDE, SIDE, *synthetic_batch(np.random.default_rng(0), BATCH, SIDE, SIDE, 2, 1)))
    return torch, args, enc, x, plan


def make_step(torch, args, stages, bn):
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    torch.manual_seed(0)
    net = Network(args, pretrained=False).to(args.device).train()
    if stages:                                              # (N = 0 makes no call: the parent commit's Network has no `freeze`)
        net.freeze(stages, bool(bn))
    return net, TrainStep(net, args)


def measure(tree, amp, configs, steps, warmup):
    torch, args, enc, x, plan = setup(tree, amp)
    out = []
    for stages, bn in configs:
        net, step = make_step(torch, args, stages, bn)
        for _ in range(warmup):
            step(x, enc.render_device(plan))
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        torch.cuda.synchronize()
        marks[0].record()
        for k in range(steps):
            loss = step(x, enc.render_device(plan))
            marks[k + 1].record()
        torch.cuda.synchronize()
        ms = sorted(marks[k].elapsed_time(marks[k + 1]) for k in range(steps))
        q = statistics.quantiles(ms, n=4)
        out.append(dict(freeze_stages=stages, freeze_bn=bool(bn), amp=bool(amp), steps=steps, step_ms_median=round(statistics.median(ms), 3),
                        step_ms_q1=round(q[0], 3), step_ms_q3=round(q[2], 3), step_ms_min=round(ms[0], 3), loss=float(loss[0])))
        del net, step
        torch.cuda.empty_cache()
    print(json.dumps(out))


def child(tree, amp, configs, steps, warmup):
    """a fresh process per measurement (its own allocator, its own warm-up); the last line of its output is the JSON"""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--measure", str(tree), "--amp", str(int(amp)), "--configs",
           ",".join(f"{n}:{b}" for n, b in configs), "--steps", str(steps), "--warmup", str(warmup)]
    done = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
    return json.loads(done.stdout.strip().splitlines()[-1])


# the three places a BatchNorm backward stands in a BasicBlock: (name, y given to the frozen form, g_out wanted, relu mode of sd_bn_bwd_apply there)
KERNEL_PAIRS = (("bn2: ReLU, masked gradient out", True, True, 3), ("bn1: ReLU", True, False, 2), ("downsample: no ReLU", False, False, 0))
KERNEL_CALLS = 10


def kernels(stages, bn):
    torch, args, enc, x, plan = setup(HERE, False)
    from structuredetector_amd import _lib as L
    lib, st = L.lib(), L.stream()
    M, Cc = BATCH * 128 * 128, 64
    for bf16 in (False, True):
        dt = torch.bfloat16 if bf16 else torch.float32
        sfx = "_bf16" if bf16 else ""
        dy, xx, y = (torch.randn(M, Cc, device="cuda").to(dt) for _ in range(3))
        mask = torch.randint(0, 16, (M * Cc // 4,), device="cuda").to(torch.uint8)
        dx, g = torch.empty_like(dy), torch.empty_like(dy)
        par = [torch.rand(Cc, device="cuda") + 0.5 for _ in range(4)]
        means = torch.randn(2 * Cc, device="cuda") * 0.01
        for _, with_y, with_g, relu in KERNEL_PAIRS:       # ten calls of the frozen form, then ten of the apply pass it replaces
            for _ in range(KERNEL_CALLS):
                L.check(getattr(lib, "sd_frozen_bn_bwd" + sfx)(dy.data_ptr(), y.data_ptr() if with_y else 0, par[0].data_ptr(), M, Cc, dx.data_ptr(),
                                                               g.data_ptr() if with_g else 0, st))
            for _ in range(KERNEL_CALLS):
                L.check(getattr(lib, "sd_bn_bwd_apply" + sfx)(dy.data_ptr(), xx.data_ptr(), mask.data_ptr() if relu == 3 else 0, relu, M, Cc,
                                                              par[0].data_ptr(), par[1].data_ptr(), par[2].data_ptr(), par[3].data_ptr(), means.data_ptr(),
                                                              dx.data_ptr(), g.data_ptr() if with_g else 0, st))
        torch.cuda.synchronize()
        del dy, xx, y, dx, g, mask
    net, step = make_step(torch, args, stages, bn)
    for _ in range(3):
        step(x, enc.render_device(plan))
    torch.cuda.synchronize()


def kernel_table(trace_csv):
    """The kernel trace of a `--kernels` run -> per precision and place: median kernel time of the frozen form and of sd_bn_bwd_apply, and the
    bytes each moves (the first 2 x 3 x 2 x KERNEL_CALLS launches of the two kernel families, in launch order)."""
    import csv
    rows = [r for r in csv.DictReader(open(trace_csv, newline="")) if "k_bn_frozen_bwd" in r["Kernel_Name"] or "k_bn_bwd_apply" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    M, Cc, out, at = BATCH * 128 * 128, 64, [], 0
    for bf16 in (False, True):
        e = M * Cc * (2 if bf16 else 4)                     # bytes of one [M][C] tensor
        for place, with_y, with_g, relu in KERNEL_PAIRS:
            us = []
            for family in ("k_bn_frozen_bwd", "k_bn_bwd_apply"):
                group = rows[at:at + KERNEL_CALLS]
                at += KERNEL_CALLS
                assert len(group) == KERNEL_CALLS and all(family in r["Kernel_Name"] for r in group), (place, family)
                us.append(statistics.median((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in group))
            out.append(dict(precision="bf16" if bf16 else "fp32", place=place, frozen_us=round(us[0], 1), bn_bwd_apply_us=round(us[1], 1),
                            frozen_bytes=e * (2 + with_y + with_g), bn_bwd_apply_bytes=e * (3 + with_g) + (M * Cc // 4 if relu == 3 else 0)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(HERE / "profiles" / "freeze_bench.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--measure", default=None)
    ap.add_argument("--amp", type=int, default=0)
    ap.add_argument("--configs", default="")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernels-stages", type=int, default=2)
    ap.add_argument("--kernels-bn", type=int, default=1)
    ap.add_argument("--kernel-table", default=None, metavar="TRACE.csv")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: the median is taken over at least 20 steps")
    if a.kernels:
        return kernels(a.kernels_stages, a.kernels_bn)
    if a.kernel_table:
        return print(json.dumps(kernel_table(a.kernel_table), indent=1))
    if a.measure:
        return measure(Path(a.measure), a.amp, [tuple(int(v) for v in c.split(":")) for c in a.configs.split(",")], a.steps, a.warmup)
    report = dict(workload=f"TrainStep, batch {BATCH}, {SIDE}x{SIDE}, synthetic targets, one GPU", timing="one pair of stream events per step after "
                  f"{a.warmup} warm-up steps; median / quartiles over {a.steps} steps; one child process per precision", table=[])
    for amp in (0, 1):
        report["table"] += child(HERE, amp, CONFIGS, a.steps, a.warmup)
    if a.parent:
        rows = []
        for amp in (0, 1):
            runs = {"parent": [], "this": []}
            for _ in range(a.rounds):                       # alternating: neither tree always runs behind the other
                runs["parent"].append(child(Path(a.parent), amp, [(0, 0)], a.steps, a.warmup)[0]["step_ms_median"])
                runs["this"].append(child(HERE, amp, [(0, 0)], a.steps, a.warmup)[0]["step_ms_median"])
            every = runs["parent"] + runs["this"]
            rows.append(dict(amp=bool(amp), parent_step_ms=runs["parent"], this_n0_step_ms=runs["this"],
                             parent_median=round(statistics.median(runs["parent"]), 3), this_median=round(statistics.median(runs["this"]), 3),
                             spread_ms=round(max(max(v) - min(v) for v in runs.values()), 3), all_min=min(every), all_max=max(every)))
        report["default_step_vs_parent"] = dict(note="medians of alternating child processes on one GPU in one session; spread_ms = the larger "
                                                "of the two trees' own round-to-round ranges", rows=rows)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(report, indent=1) + "\n")
    for r in report["table"]:
        print(f"{'amp ' if r['amp'] else 'fp32'} N={r['freeze_stages']} bn={int(r['freeze_bn'])}: {r['step_ms_median']:.3f} ms "
              f"[{r['step_ms_q1']:.3f}, {r['step_ms_q3']:.3f}]")
    for r in report.get("default_step_vs_parent", {}).get("rows", []):
        print(f"{'amp ' if r['amp'] else 'fp32'} default step: parent {r['parent_step_ms']} this {r['this_n0_step_ms']} spread {r['spread_ms']} ms")


if __name__ == "__main__":
    main()
