#!/usr/bin/env python3
"""GPU time of the preprocess call with and without the letterbox (`--keep_aspect`), bs = 64, 2448x2048 sources -> 512x512: packed and list
forms, plain (resize + flips-free Normalize) and with jitter + flips.  Device events around `--reps` calls, `--rounds` rounds after a warm-up
of every shape; per row the best round of the letterbox call beside the best round of the stretched ("plain") call on the same sources, and
the spread (min .. max over the rounds) of the plain call, which is what a difference has to exceed to mean anything.  The letterbox
resamples 512 x 428 instead of 512 x 512 output pixels and writes the same frame.  Writes one JSON document (default
profiles/letterbox_bench.json)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from structuredetector_amd.data import letterbox_geometry, preprocess_image_list, preprocess_images  # noqa: E402
from structuredetector_amd.data.augment import jitter_words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--label", type=str, default="")
ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "letterbox_bench.json")
opt = ap.parse_args()

dev = torch.device("cuda")
rng = np.random.default_rng(0)
B, size, (H, W) = opt.batch, (512, 512), (2048, 2448)
box = letterbox_geometry((W, H), size)
flips = [int(v) for v in rng.integers(0, 4, B)]
words, factors = zip(*(jitter_words(list(rng.permutation(4)), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.85, 1.15),
                                    rng.uniform(-0.05, 0.05)) for _ in range(B)))
jitter = (list(words), list(factors))


def timed(fn):
    """us per call of every round: (best, worst)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(opt.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(opt.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / opt.reps * 1e3)
    return min(rounds), max(rounds)


x = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
table = torch.tensor([x[b].data_ptr() for b in range(B)], dtype=torch.int64, device=dev)
rows = []
for form in ("packed", "list"):
    for chain, kw in (("plain", {}), ("jitter_flips", dict(flips=flips, jitter=jitter))):
        if form == "packed":
            call = lambda **extra: preprocess_images(x, size, **kw, **extra)
        else:
            call = lambda **extra: preprocess_image_list(table, H, W, size, **kw, **extra)
        plain_best, plain_worst = timed(call)
        box_best, box_worst = timed(lambda: call(letterbox=box))
        again_best, again_worst = timed(call)                                   # the plain call once more: its run-to-run spread
        lo, hi = min(plain_best, again_best), max(plain_worst, again_worst)
        row = {"source": f"{W}x{H}", "out": "512x512", "inner": f"{box[0]}x{box[1]}", "batch": B, "form": form, "chain": chain,
               "plain_us_per_call": round(lo, 1), "plain_spread_us": [round(lo, 1), round(hi, 1)],
               "letterbox_us_per_call": round(box_best, 1), "letterbox_spread_us": [round(box_best, 1), round(box_worst, 1)],
               "letterbox_minus_plain_us": round(box_best - lo, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
doc = {"tool": "tools/letterbox_bench.py", "label": opt.label, "device": torch.cuda.get_device_name(0), "reps": opt.reps, "rounds": opt.rounds,
       "rows": rows}
opt.out.parent.mkdir(parents=True, exist_ok=True)
opt.out.write_text(json.dumps(doc, indent=1) + "\n")
