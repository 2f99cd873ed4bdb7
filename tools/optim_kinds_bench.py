#!/usr/bin/env python3
"""The three update rules on the production flat buffer (the ResNet-34 + FPN-128 network: 21.85 M floats), decay + clipping + EMA on, in
one process:

  sd_optim_groups_step   Adam in the groups form -- the yardstick
  sd_sgd_step            momentum 0.9 (one state buffer)
  sd_lamb_step           both of its launches together (k_lamb_moments, k_lamb_apply)

All read the same partials of one `sd_grad_sumsq` call and the 14 groups of `Network.optim_groups()`; only the update is timed: one pair of
stream events per call, the entry points alternating, `--launches` timed calls each after `--warmup` of each.  Then the whole `TrainStep`
(batch 64, 512x512, fp32 and --amp) with the options on, per optimizer, beside the plain step.

The tool also runs on a tree from before the optimizer choice: there it times what exists (sd_optim_groups_step, the plain step and the
step with the options).  `--parent-json FILE` puts such a report into this one under "parent" -- the yardstick of the parent commit.

  optim_kinds_bench.py [--out profiles/optim_kinds_bench.json] [--launches 100] [--warmup 10] [--steps 20] [--step-warmup 5] [--no-steps]
                       [--parent-json FILE]"""
import argparse
import ctypes as C
import inspect
import json
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(HERE))
BATCH, SIDE = 64, 512
LR, B1, B2, EPS, WD, MAX_NORM, EMA_DECAY, MOMENTUM = 1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, 0.999, 0.9
# fp32 buffer passes of the update, EMA on: read + write of p, state buffers and EMA, one read of grad (LAMB: both launches)
PASSES = {"sd_optim_groups_step": 9, "sd_sgd_step": 7, "sd_lamb_step": 12}      # LAMB: 6 (p, g read; m, v read + written) + 6 (m, v read; p, EMA both)


def summary(us):
    us = sorted(us)
    q = statistics.quantiles(us, n=4)
    return dict(median=round(statistics.median(us), 2), min=round(us[0], 2), max=round(us[-1], 2), q1=round(q[0], 2), q3=round(q[2], 2), launches=len(us))


def kernels(torch, args, launches, warmup):
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model import Network
    lib, dev = L.lib(), args.device
    net = Network(args, pretrained=False).to(dev)
    n = net.flat_params.numel()
    ids, groups = net.optim_groups()
    ids = ids.to(dev)
    lr_mul = (C.c_float * len(groups))(*(1.0 for _ in groups))
    wd_mul = (C.c_float * len(groups))(*(float(decayed) for _, decayed in groups))
    names = [name for name in PASSES if name in L.declared_symbols()]
    table = None
    if "sd_lamb_step" in names:                              # the network's own slot table, built and uploaded once
        slots = net.optim_slots()
        count = len(slots)
        lo, hi = (C.c_int64 * count)(*(s[0] for s in slots)), (C.c_int64 * count)(*(s[1] for s in slots))
        adapt = (C.c_ubyte * count)(*(int(s[2]) for s in slots))
        need, nblocks = C.c_size_t(), C.c_int()
        L.check(lib.sd_lamb_table_build(lo, hi, adapt, count, n, None, 0, C.byref(need), C.byref(nblocks)), "sd_lamb_table_build")
        host = torch.zeros(need.value // 4, dtype=torch.int32)
        L.check(lib.sd_lamb_table_build(lo, hi, adapt, count, n, host.data_ptr(), need.value, None, None), "sd_lamb_table_build")
        ws = torch.empty(lib.sd_lamb_workspace_bytes(nblocks.value) // 8, dtype=torch.float64, device=dev)
        table = (host.to(dev), count, nblocks.value, ws)
    gen = torch.Generator(dev).manual_seed(0)
    grad = torch.randn(n, device=dev, generator=gen) * 1e-3
    partials = torch.empty(lib.sd_grad_sumsq_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
    L.check(lib.sd_grad_sumsq(grad.data_ptr(), n, partials.data_ptr(), partials.numel() * 8, L.stream()), "sd_grad_sumsq")
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    # a set of buffers per entry point: none finds another's lines in the caches
    state = {name: [net.flat_params.detach().clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), net.flat_params.detach().clone()]
             for name in names}
    del net

    def launch(name, step):
        p, m, v, ema = state[name]
        groups_form = (1.0, WD, ids.data_ptr(), lr_mul, wd_mul, len(groups), MAX_NORM, partials.data_ptr(), partials.numel(), ema.data_ptr(), EMA_DECAY,
                       status.data_ptr())
        if name == "sd_optim_groups_step":
            L.check(lib.sd_optim_groups_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, LR, B1, B2, EPS, *groups_form, L.stream()), name)
        elif name == "sd_sgd_step":
            L.check(lib.sd_sgd_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), n, LR, MOMENTUM, 0, *groups_form, L.stream()), name)
        else:
            tab, nslots, nblocks, ws = table
            L.check(lib.sd_lamb_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, LR, B1, B2, EPS, *groups_form, tab.data_ptr(),
                                     nslots, nblocks, ws.data_ptr(), ws.numel() * 8, L.stream()), name)

    times = {name: [] for name in names}
    for k in range(warmup + launches):
        for name in names:                                  # alternating: none always runs behind the same other
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(name, k + 1)
            e1.record()
            e1.synchronize()
            if k >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert int(status[2]) == 0, "a launch was skipped: the norm was not finite"
    out = {}
    for name, us in times.items():
        moved = n * 4 * PASSES[name] + n // 4 * (2 if name == "sd_lamb_step" else 1)         # + the id bytes, once per launch
        out[name] = dict(summary(us), buffer_passes=PASSES[name], bytes_moved=moved, GBps_at_median=round(moved / statistics.median(us) / 1e3, 1))
    base = out["sd_optim_groups_step"]
    for name, r in out.items():
        r["time_ratio_to_groups"] = round(r["median"] / base["median"], 3)
        r["traffic_ratio_to_groups"] = round(r["bytes_moved"] / base["bytes_moved"], 3)
    report = dict(n=n, groups=len(groups), options=dict(weight_decay=WD, clip_grad_norm=MAX_NORM, ema_decay=EMA_DECAY, momentum=MOMENTUM), us=out)
    if table is not None:
        report["lamb_table"] = dict(slots=table[1], blocks=table[2], table_bytes=table[0].numel() * 4, workspace_bytes=table[3].numel() * 8)
    return report


def steps(torch, args, count, warmup):
    import numpy as np
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    dev = args.device
    options = dict(weight_decay=WD, clip_grad_norm=MAX_NORM, ema_decay=EMA_DECAY)
    kinds = [("adam, plain", {}), ("adam", options)]
    if "optimizer" in inspect.signature(TrainStep).parameters:
        kinds += [("sgd", dict(options, optimizer="sgd", momentum=MOMENTUM)), ("lamb", dict(options, optimizer="lamb"))]
    x = torch.randn(BATCH, 3, SIDE, SIDE, device=dev, generator=torch.Generator(dev).manual_seed(0))
    out = []
    for amp in (False, True):
        args.use_amp = amp
        enc = Encode(args)
        plan = enc.upload(enc.plan(SIDE, SIDE, *synthetic_batch(np.random.default_rng(0), BATCH, SIDE, SIDE, 2, 1)))
        for name, kw in kinds:
            torch.manual_seed(0)
            net = Network(args, pretrained=False).to(dev).train()
            step = TrainStep(net, args, **kw)
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
            out.append(dict(amp=amp, optimizer=name, steps=count, step_ms_median=round(statistics.median(ms), 3), step_ms_min=round(ms[0], 3),
                            step_ms_max=round(ms[-1], 3)))
            del net, step
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(HERE / "profiles" / "optim_kinds_bench.json"))
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--parent-json", default=None, help="a report of this tool run on the parent commit: embedded under 'parent'")
    a = ap.parse_args()
    if a.launches < 50:
        ap.error("--launches: the median is taken over at least 50 launches of each entry point")
    import torch
    from bench import make_args
    args = make_args(torch.device("cuda"))
    report = dict(timing=f"one pair of stream events per call, the entry points alternating, {a.launches} timed calls each after {a.warmup}; "
                  "microseconds; sd_lamb_step: both launches", kernels=kernels(torch, args, a.launches, a.warmup))
    if not a.no_steps:
        report["steps"] = dict(workload=f"TrainStep, batch {BATCH}, {SIDE}x{SIDE}, synthetic targets; 'adam, plain': no option, every other row "
                               f"weight_decay {WD}, clip_grad_norm {MAX_NORM}, ema_decay {EMA_DECAY}",
                               timing=f"one pair of stream events per step after {a.step_warmup} warm-up steps", table=steps(torch, args, a.steps, a.step_warmup))
    if a.parent_json:
        report["parent"] = json.loads(Path(a.parent_json).read_text())
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(report, indent=1) + "\n")
    for name, r in report["kernels"]["us"].items():
        print(f"{name}: median {r['median']} us [{r['min']}, {r['max']}] {r['GBps_at_median']} GB/s, x{r['time_ratio_to_groups']} of the groups step "
              f"(traffic x{r['traffic_ratio_to_groups']})")
    for r in report.get("steps", {}).get("table", []):
        print(f"{'amp ' if r['amp'] else 'fp32'} {r['optimizer']}: {r['step_ms_median']} ms [{r['step_ms_min']}, {r['step_ms_max']}]")


if __name__ == "__main__":
    main()
