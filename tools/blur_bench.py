#!/usr/bin/env python3
"""GPU time of the gaussian blur augmentation (`train --aug_blur`), bs = 64, network input 512x512.  Device events around `--reps` calls,
`--rounds` rounds after a warm-up of every variant; us per call, best round, and the spread (min .. max over the rounds).

1. `sd_blur_u8` alone on (64, 512, 512, 3) bytes for the box radii 1 (r = 2) and SD_BLUR_MAX_RADIUS (r = 8), every image blurred, beside its
   HBM floor: the image bytes read once and written once per direction launched (two launches), at the copy rate `tools/hbm_rw_micro.py`
   measures (a 1 GiB fp32 `copy_`, read + write), taken here in the same process.
2. The training chain (ColorJitter + flips, packed and pointer-list, 2448x2048 sources) with the blur table `--aug_blur 2` draws (an image is
   blurred when u0 < 0.5, r = 2 u1) beside the same chain without the flag, which is timed before and after: its own run-to-run spread is
   what a flag-off difference has to exceed to mean anything.

`--off-only` times just the flag-off chain through the entry points that exist without the feature; with `--package-root` it imports the
package from another checkout (the parent commit, built), and `--parent-json` merges that run's rows into this one's document.
Writes one JSON document (default profiles/blur_bench.json)."""
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
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--package-root", type=Path, default=Path(__file__).resolve().parent.parent)
ap.add_argument("--parent-json", type=Path, default=None)
ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "blur_bench.json")
opt = ap.parse_args()

sys.path.insert(0, str(opt.package_root.resolve()))
from structuredetector_amd.data import preprocess_image_list, preprocess_images  # noqa: E402
from structuredetector_amd.data.augment import jitter_words  # noqa: E402

dev = torch.device("cuda")
rng = np.random.default_rng(0)
B, size, (H, W) = opt.batch, (512, 512), (2048, 2448)
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


doc = {"tool": "tools/blur_bench.py", "label": opt.label, "device": torch.cuda.get_device_name(0), "reps": opt.reps, "rounds": opt.rounds,
       "batch": B, "out": "512x512"}

if not opt.off_only:
    from structuredetector_amd.data import blur_box_params, blur_images  # noqa: E402
    a = torch.empty(1 << 28, device=dev)
    b = torch.empty(1 << 28, device=dev)
    best, worst = timed(lambda: b.copy_(a), reps=5)
    copy_tbs = 2 * (1 << 30) / 1e12 / (best * 1e-6)
    doc["hbm_copy"] = {"what": "1 GiB fp32 copy_ (read + write), the measurement of tools/hbm_rw_micro.py", "us": round(best, 1),
                       "tb_per_s": round(copy_tbs, 3)}
    print(json.dumps(doc["hbm_copy"]), flush=True)
    del a, b
    img = torch.from_numpy(rng.integers(0, 256, (B, size[1], size[0], 3), dtype=np.uint8)).to(dev)
    floor_bytes = 2 * 2 * img.numel()                                           # two directions, each one read and one write of the images
    doc["stage"] = []
    from structuredetector_amd import _lib as L  # noqa: E402
    lib = L.lib()
    dst = torch.empty_like(img)
    ws = L.workspace(lib.sd_blur_workspace_bytes(B, size[1], size[0]), img.device)
    for r in (2.0, 8.0):
        table = [blur_box_params(r)] * B
        rows_dev = torch.tensor(table, dtype=torch.int32, device=dev)           # uploaded once: the timed call is the two launches alone
        assert torch.equal(blur_images(img, table), blur_images(img, table))
        best, worst = timed(lambda: L.check(lib.sd_blur_u8(img.data_ptr(), dst.data_ptr(), B, size[1], size[0], rows_dev.data_ptr(), ws.data_ptr(),
                                                           ws.numel(), L.stream()), "sd_blur_u8"), reps=50)
        floor_us = floor_bytes / (copy_tbs * 1e12) * 1e6
        row = {"entry": "sd_blur_u8", "gaussian_radius": r, "box_radius": table[0][0], "us_per_call": round(best, 1),
               "spread_us": [round(best, 1), round(worst, 1)], "hbm_floor_bytes": floor_bytes, "hbm_floor_us_at_copy_rate": round(floor_us, 1),
               "reached_fraction_of_floor": round(floor_us / best, 3), "tb_per_s": round(floor_bytes / 1e12 / (best * 1e-6), 3)}
        doc["stage"].append(row)
        print(json.dumps(row), flush=True)
    del img, dst
    radii = [float(2.0 * u1) if u0 < 0.5 else 0.0 for u0, u1 in draws]
    blur = [blur_box_params(r) for r in radii]
    doc["chain_blur_table"] = {"flag": 2.0, "blurred": int(sum(r > 0 for r in radii)), "box_radius_counts": {str(k): sum(1 for t in blur if t[0] == k and t[2])
                                                                                                      for k in sorted({t[0] for t in blur})}}

x = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
table = torch.tensor([x[i].data_ptr() for i in range(B)], dtype=torch.int64, device=dev)
rows = []
for form in ("packed", "list"):
    kw = dict(flips=flips, jitter=jitter)
    if form == "packed":
        call = lambda **extra: preprocess_images(x, size, **kw, **extra)
    else:
        call = lambda **extra: preprocess_image_list(table, H, W, size, **kw, **extra)
    off_best, off_worst = timed(call)
    row = {"source": f"{W}x{H}", "form": form, "chain": "jitter_flips"}
    if not opt.off_only:
        on_best, on_worst = timed(lambda: call(blur=blur))
        again_best, again_worst = timed(call)                                   # the flag-off call once more: its run-to-run spread
        off_best, off_worst = min(off_best, again_best), max(off_worst, again_worst)
        row.update({"aug_blur_2_us_per_call": round(on_best, 1), "aug_blur_2_spread_us": [round(on_best, 1), round(on_worst, 1)],
                    "blur_minus_off_us": round(on_best - off_best, 1)})
    row.update({"off_us_per_call": round(off_best, 1), "off_spread_us": [round(off_best, 1), round(off_worst, 1)]})
    rows.append(row)
    print(json.dumps(row), flush=True)
doc["chain"] = rows
if opt.parent_json is not None and opt.parent_json.exists():
    parent = json.loads(opt.parent_json.read_text())
    doc["chain_at_parent_commit"] = {"label": parent.get("label", ""), "rows": parent["chain"]}
opt.out.parent.mkdir(parents=True, exist_ok=True)
opt.out.write_text(json.dumps(doc, indent=1) + "\n")
