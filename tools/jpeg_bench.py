#!/usr/bin/env python3
"""GPU time of the JPEG compression augmentation (`train --aug_jpeg`), bs = 64, network input 512x512.  Device events around `--reps` calls,
`--rounds` rounds after a warm-up of every variant; us per call, best round, and the spread (min .. max over the rounds).

1. `sd_jpeg_u8` alone on (64, 512, 512, 3) bytes at the qualities 10 and 90, every image compressed, beside
   - a device copy of the same bytes (`copy_` of the image tensor: 3 B/px read + 3 B/px written), timed in the same process, and
   - its HBM floor of 9 B/px -- the image read and the planes written (3 + 1.5), the planes read and the image written (1.5 + 3) -- at the
     copy rate of a 1 GiB fp32 `copy_` (read + write; the measurement of `tools/hbm_rw_micro.py`), taken here in the same process.
2. The training chain (ColorJitter + flips, packed and pointer-list, 2448x2048 sources) with the table `--aug_jpeg 30` draws (an image is
   compressed when u0 < 0.5, at a quality uniform in [30, 95]) beside the same chain without the flag, which is the previous path (a null
   table never reaches the new code) and is timed before and after: its own run-to-run spread is what a difference has to exceed.

Writes one JSON document (default profiles/jpeg_bench.json)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--label", type=str, default="")
ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "jpeg_bench.json")
opt = ap.parse_args()

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from structuredetector_amd import _lib as L  # noqa: E402
from structuredetector_amd.data import jpeg_images, jpeg_rows, preprocess_image_list, preprocess_images  # noqa: E402
from structuredetector_amd.data.augment import jitter_words  # noqa: E402

dev = torch.device("cuda")
rng = np.random.default_rng(0)
B, size, (H, W) = opt.batch, (512, 512), (2048, 2448)
QMIN = 30
flips = [int(v) for v in rng.integers(0, 4, B)]
words, factors = zip(*(jitter_words(list(rng.permutation(4)), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.85, 1.15),
                                    rng.uniform(-0.05, 0.05)) for _ in range(B)))
jitter = (list(words), list(factors))
draws = rng.uniform(0, 1, (B, 2))


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


doc = {"tool": "tools/jpeg_bench.py", "label": opt.label, "device": torch.cuda.get_device_name(0), "reps": opt.reps, "rounds": opt.rounds,
       "batch": B, "out": "512x512"}

a = torch.empty(1 << 28, device=dev)
b = torch.empty(1 << 28, device=dev)
best, worst = timed(lambda: b.copy_(a), reps=5)
copy_tbs = 2 * (1 << 30) / 1e12 / (best * 1e-6)
doc["hbm_copy"] = {"what": "1 GiB fp32 copy_ (read + write), the measurement of tools/hbm_rw_micro.py", "us": round(best, 1), "tb_per_s": round(copy_tbs, 3)}
print(json.dumps(doc["hbm_copy"]), flush=True)
del a, b

# smooth content plus noise: what a resized photograph looks like to the quantiser (pure noise keeps every coefficient alive)
yy, xx = np.mgrid[0:size[1], 0:size[0]].astype(np.float32)
base = np.stack([127.5 + 100 * np.sin(xx / 37 + yy / 53), 127.5 + 100 * np.cos(xx / 29), 255 * yy / size[1]], axis=-1)
img = torch.from_numpy(np.clip(base[None] + rng.normal(0, 12, (B, size[1], size[0], 3)), 0, 255).astype(np.uint8)).to(dev)
dst = torch.empty_like(img)
best, worst = timed(lambda: dst.copy_(img), reps=50)
doc["image_copy"] = {"what": "copy_ of the (64, 512, 512, 3) uint8 batch: 6 B/px", "us_per_call": round(best, 1), "spread_us": [round(best, 1), round(worst, 1)],
                     "tb_per_s": round(2 * img.numel() / 1e12 / (best * 1e-6), 3)}
print(json.dumps(doc["image_copy"]), flush=True)
copy_us = best
floor_bytes = 3 * img.numel()                                                   # 9 B/px
lib = L.lib()
ws = L.workspace(lib.sd_jpeg_workspace_bytes(B, size[1], size[0]), img.device)
doc["stage"] = []
for q in (10, 90):
    table = jpeg_rows([q] * B)
    rows_dev = torch.tensor(table, dtype=torch.int32, device=dev)               # uploaded once: the timed call is the two launches alone
    assert torch.equal(jpeg_images(img, table), jpeg_images(img, table))
    best, worst = timed(lambda: L.check(lib.sd_jpeg_u8(img.data_ptr(), dst.data_ptr(), B, size[1], size[0], rows_dev.data_ptr(), ws.data_ptr(),
                                                       ws.numel(), L.stream()), "sd_jpeg_u8"), reps=50)
    floor_us = floor_bytes / (copy_tbs * 1e12) * 1e6
    row = {"entry": "sd_jpeg_u8", "quality": q, "us_per_call": round(best, 1), "spread_us": [round(best, 1), round(worst, 1)],
           "image_copy_us": round(copy_us, 1), "times_the_image_copy": round(best / copy_us, 2), "hbm_floor_bytes": floor_bytes,
           "hbm_floor_us_at_copy_rate": round(floor_us, 1), "reached_fraction_of_floor": round(floor_us / best, 3),
           "tb_per_s": round(floor_bytes / 1e12 / (best * 1e-6), 3)}
    doc["stage"].append(row)
    print(json.dumps(row), flush=True)
del img, dst

qualities = [min(95, QMIN + int(u1 * (96 - QMIN))) if u0 < 0.5 else 0 for u0, u1 in draws]
jpeg = jpeg_rows(qualities)
doc["chain_jpeg_table"] = {"flag": QMIN, "compressed": int(sum(q > 0 for q in qualities)), "qualities": sorted(q for q in qualities if q)}

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
    on_best, on_worst = timed(lambda: call(jpeg=jpeg))
    again_best, again_worst = timed(call)                                       # the flag-off call once more: its run-to-run spread
    off_best, off_worst = min(off_best, again_best), max(off_worst, again_worst)
    row = {"source": f"{W}x{H}", "form": form, "chain": "jitter_flips", "aug_jpeg_30_us_per_call": round(on_best, 1),
           "aug_jpeg_30_spread_us": [round(on_best, 1), round(on_worst, 1)], "jpeg_minus_off_us": round(on_best - off_best, 1),
           "off_us_per_call": round(off_best, 1), "off_spread_us": [round(off_best, 1), round(off_worst, 1)]}
    rows.append(row)
    print(json.dumps(row), flush=True)
doc["chain"] = rows
opt.out.parent.mkdir(parents=True, exist_ok=True)
opt.out.write_text(json.dumps(doc, indent=1) + "\n")
