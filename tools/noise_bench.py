#!/usr/bin/env python3
"""GPU time of the sensor-noise stage (`train --aug_noise / --aug_noise_shot`), bs = 64, network input 512x512.  Device events around
`--reps` calls, `--rounds` rounds after a warm-up of every variant; us per call, best round, and the spread (min .. max).

1. `sd_noise_u8` on (64, 512, 512, 3) random bytes into a second buffer (the chain runs it in place: the same 3 B/px read + 3 B/px written,
   but here every call sees the same content), for the tables read-only (sigma 4), shot-only (gain 0.5), both (sigma 6, gain 0.5) and half
   (every other image an identity row, which in place costs nothing but here is a copy); beside
   - a device copy of the same bytes (`copy_` of the image tensor: the same 6 B/px), timed in the same process, and
   - the stage's arithmetic: 10 rounds x 4 32-bit multiplies per Philox call, one call per four bytes, as a count (no peak rate is claimed).
   With `--stage_only TABLE` this tool runs that one variant `--reps` times and writes nothing (for a kernel trace, a run of its own).
2. The training chain (ColorJitter + flips, packed and pointer-list, 2448x2048 sources) with the table that `--aug_noise 6 --aug_noise_shot
   0.5` draws beside the same chain without the flags, which is the previous path (a null table never reaches the new code) and is timed
   before and after: its own run-to-run spread is what a difference has to exceed.

Writes one JSON document (default profiles/noise_bench.json)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--label", type=str, default="")
ap.add_argument("--stage_only", type=str, default="", metavar="TABLE", help="run one variant of part 1 and stop (for a kernel trace)")
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "noise_bench.json")
opt = ap.parse_args()

sys.path.insert(0, str(ROOT))
from structuredetector_amd import _lib as L  # noqa: E402
from structuredetector_amd.data import noise_images, noise_rows, preprocess_image_list, preprocess_images  # noqa: E402
from structuredetector_amd.data.augment import jitter_words  # noqa: E402

dev = torch.device("cuda")
rng = np.random.default_rng(0)
B, size, (H, W) = opt.batch, (512, 512), (2048, 2448)
READ, SHOT = 6.0, 0.5
n_bytes = 3 * size[0] * size[1]


def timed(fn, reps=None):
    """us per call of every round: (best, worst)."""
    reps = reps or opt.reps
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(opt.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / reps * 1e3)
    return min(rounds), max(rounds)


keys = [(int(k0), int(k1)) for k0, k1 in rng.integers(0, 2 ** 32, (B, 2))]
TABLES = {"read": [(k0, k1, 4.0, 0.0) for k0, k1 in keys], "shot": [(k0, k1, 0.0, 0.5) for k0, k1 in keys],
          "both": [(k0, k1, READ, SHOT) for k0, k1 in keys],
          "half": [(k0, k1, READ, SHOT) if i % 2 == 0 else (k0, k1, 0.0, 0.0) for i, (k0, k1) in enumerate(keys)]}
lib = L.lib()
src = torch.from_numpy(rng.integers(0, 256, (B, size[1], size[0], 3), dtype=np.uint8)).to(dev)
dst = torch.empty_like(src)


def stage_call(rows_dev):
    """The one launch alone: the table is on the device already."""
    return lambda: L.check(lib.sd_noise_u8(src.data_ptr(), dst.data_ptr(), B, size[1], size[0], rows_dev.data_ptr(), L.stream()), "sd_noise_u8")


if opt.stage_only:
    call = stage_call(torch.tensor(noise_rows(TABLES[opt.stage_only]), dtype=torch.int32, device=dev))
    for _ in range(opt.reps):
        call()
    torch.cuda.synchronize()
    sys.exit(0)

doc = {"tool": "tools/noise_bench.py", "label": opt.label, "device": torch.cuda.get_device_name(0), "reps": opt.reps, "rounds": opt.rounds,
       "batch": B, "out": "512x512"}

copy_best, copy_worst = timed(lambda: dst.copy_(src), reps=50)
doc["image_copy"] = {"what": "copy_ of the (B, 512, 512, 3) uint8 tensor: 3 B/px read + 3 B/px written", "us": round(copy_best, 1),
                     "spread_us": [round(copy_best, 1), round(copy_worst, 1)], "tb_per_s": round(2 * B * n_bytes / 1e12 / (copy_best * 1e-6), 3)}
print(json.dumps(doc["image_copy"]), flush=True)

doc["stage"] = []
for name, draws in TABLES.items():
    table = noise_rows(draws)
    rows_dev = torch.tensor(table, dtype=torch.int32, device=dev)
    assert torch.equal(noise_images(src, table), noise_images(src, table))
    best, worst = timed(stage_call(rows_dev), reps=50)
    selected = sum(s > 0 or g > 0 for _, _, s, g in draws)
    calls = selected * n_bytes // 4
    row = {"entry": "sd_noise_u8 (out of place)", "table": name, "selected": selected, "us_per_call": round(best, 1),
           "spread_us": [round(best, 1), round(worst, 1)], "image_copy_us": round(copy_best, 1), "times_the_image_copy": round(best / copy_best, 2),
           "bytes_moved": 2 * B * n_bytes, "tb_per_s": round(2 * B * n_bytes / 1e12 / (best * 1e-6), 3), "philox_calls": calls,
           "mul32_count": 40 * calls, "mul32_per_ns": round(40 * calls / (best * 1e3), 1)}
    doc["stage"].append(row)
    print(json.dumps(row), flush=True)
del src, dst

flips = [int(v) for v in rng.integers(0, 4, B)]
words, factors = zip(*(jitter_words(list(rng.permutation(4)), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.85, 1.15),
                                    rng.uniform(-0.05, 0.05)) for _ in range(B)))
jitter = (list(words), list(factors))
u = rng.uniform(0, 1, (B, 3))
draws = [(k0, k1, u1 * READ, u2 * SHOT) if u0 < 0.5 else (k0, k1, 0.0, 0.0) for (u0, u1, u2), (k0, k1) in zip(u, keys)]
noise = noise_rows(draws)
doc["chain_noise_table"] = {"aug_noise": READ, "aug_noise_shot": SHOT, "noised": int(sum(s > 0 or g > 0 for _, _, s, g in draws))}

x = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
pointers = torch.tensor([x[i].data_ptr() for i in range(B)], dtype=torch.int64, device=dev)
rows = []
for form in ("packed", "list"):
    kw = dict(flips=flips, jitter=jitter)
    if form == "packed":
        call = lambda **extra: preprocess_images(x, size, **kw, **extra)
    else:
        call = lambda **extra: preprocess_image_list(pointers, H, W, size, **kw, **extra)
    off_best, off_worst = timed(call)
    on_best, on_worst = timed(lambda: call(noise=noise))
    again_best, again_worst = timed(call)                                       # the flag-off call once more: its run-to-run spread
    off_best, off_worst = min(off_best, again_best), max(off_worst, again_worst)
    row = {"source": f"{W}x{H}", "form": form, "chain": "jitter_flips", "noise_us_per_call": round(on_best, 1),
           "noise_spread_us": [round(on_best, 1), round(on_worst, 1)], "noise_minus_off_us": round(on_best - off_best, 1),
           "off_us_per_call": round(off_best, 1), "off_spread_us": [round(off_best, 1), round(off_worst, 1)]}
    rows.append(row)
    print(json.dumps(row), flush=True)
doc["chain"] = rows
opt.out.parent.mkdir(parents=True, exist_ok=True)
opt.out.write_text(json.dumps(doc, indent=1) + "\n")
