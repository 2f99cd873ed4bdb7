#!/usr/bin/env python3
"""Cost of the synchronized-BatchNorm split on ONE GPU (world 1: the split statistics finish, no collective), DESIGN section 7.

    python tools/sync_bn_bench.py [--batch 64] [--size 512] [--rounds 3] [--steps 20] [--warmup 5] [--out profiles/x.json]
        fp32 and --amp: the default step and the sync_bn=True step alternate in one process (same network, two TrainSteps), each
        round times `--steps` steps of one mode between stream events; the JSON line holds the medians over the rounds.
    python tools/sync_bn_bench.py --trace-steps 3 --mode {default,sync} [--amp]
        only that many steps of one mode (for `rocprofv3 --kernel-trace --stats`, one run per mode);
    python tools/sync_bn_bench.py --count-launches kernel_trace.csv
        launches of the last complete step in such a trace (between the last two Adam launches, as tools/trace_small_launches.sh).
What N > 1 ranks add (up to 78 latency-bound all-reduces of <= 2 * 512 + 1 doubles per step, waits behind gradient buckets) is
not measurable on one GPU and not part of these figures."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def count_launches(csv_path):
    import csv
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    adam = [i for i, r in enumerate(rows) if "k_adam" in r["Kernel_Name"]]
    if len(adam) < 2:
        raise SystemExit("need a trace of at least two steps")
    step = rows[adam[-2] + 1:adam[-1] + 1]
    return {"launches_last_step": len(step), "launches_total": len(rows), "steps_in_trace": len(adam)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--mode", choices=("default", "sync"), default="default")
    ap.add_argument("--amp", action="store_true")
    ap.add_argument("--count-launches", type=str, default=None)
    a = ap.parse_args()
    if a.count_launches:
        print(json.dumps(count_launches(a.count_launches)))
        return

    import numpy as np
    import torch

    from bench import make_args
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    dev = torch.device("cuda")
    B, img = a.batch, a.size
    x = torch.randn(B, 3, img, img, device=dev, generator=torch.Generator(dev).manual_seed(0))

    def build(amp):
        args = make_args(dev)
        args.use_amp = amp
        net = Network(args, pretrained=False).to(dev).train()
        enc = Encode(args)
        tgt = enc.render(enc.plan(img, img, *synthetic_batch(np.random.default_rng(0), B, img, img, 2, 1)), dev)
        return net, {"default": TrainStep(net, args), "sync": TrainStep(net, args, sync_bn=True)}, tgt

    if a.trace_steps:
        net, steps, tgt = build(a.amp)
        for _ in range(a.trace_steps):
            steps[a.mode](x, tgt)
        torch.cuda.synchronize()
        print(json.dumps({"mode": a.mode, "amp": a.amp, "steps": a.trace_steps}))
        return

    rec = {"what": "sync_bn split statistics finish at world 1 (no collective) vs the default step", "batch": B, "size": img,
           "rounds": a.rounds, "steps_per_round": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for amp in (False, True):
        net, steps, tgt = build(amp)
        for mode in ("default", "sync"):
            for _ in range(a.warmup):
                steps[mode](x, tgt)
        torch.cuda.synchronize()
        ms = {"default": [], "sync": []}
        for _ in range(a.rounds):
            for mode in ("default", "sync"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    steps[mode](x, tgt)
                e1.record()
                e1.synchronize()
                ms[mode].append(e0.elapsed_time(e1) / a.steps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec["amp" if amp else "fp32"] = {"ms_per_step_default": round(med["default"], 3), "ms_per_step_sync": round(med["sync"], 3),
                                          "overhead_pct": round(100.0 * (med["sync"] / med["default"] - 1.0), 2),
                                          "rounds_default_ms": [round(v, 3) for v in ms["default"]],
                                          "rounds_sync_ms": [round(v, 3) for v in ms["sync"]]}
        del net, steps
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
