#!/usr/bin/env python3
"""GPU time of the preprocess call with and without the mosaic, bs = 64: 512x512 -> 512x512 and 2448x2048 -> 512x512, jitter on and off,
packed and list forms (the rows of tools/affine_bench.py).  Device events around `--reps` calls, `--rounds` rounds after a warm-up of every
shape; within a round the variants of one row run one after the other, so a round's differences see the same machine state.  Beside each
row with the mosaic: the extra time over the same row without it (best round of each) and the HBM floor of the added launch (k_mosaic_u8:
3 B read + 3 B written per pixel; k_mosaic_norm: 3 B read + 12 B written) at `--hbm_tbs` TB/s (the copy rate of tools/hbm_rw_micro.py).
The yardstick for k_mosaic_u8 is k_affine_u8 in the same process on the same batch (jitter rows: both feed the same jitter launches), per
round the extra time of each over the row without either:
  affine_half   the warp with the mosaic's own 1/2-zoom matrix of tile 3 (one matrix per image: it samples a quarter of the canvas, the
                rest is fill and costs no loads -- the mosaic samples 9/16 to all of it)
  affine_full   the warp with a half-pixel shift [1, 0, .5, 0, 1, .5]: the mosaic's 2 x 2 taps on (nearly) every pixel of the canvas
`yardstick` in the output holds the per-round extras, their medians and the spread (max - min) / median of each.
`--mosaic off` times only the rows without it: that also runs on a commit that has no mosaic, for the comparison with the parent.
Writes one JSON document (default profiles/mosaic_bench.json)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from structuredetector_amd.data import preprocess_image_list, preprocess_images  # noqa: E402
from structuredetector_amd.data.augment import jitter_words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mosaic", choices=["both", "off"], default="both")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--hbm_tbs", type=float, default=0.0, help="measured HBM copy rate in TB/s for the floors (0 = leave them out)")
ap.add_argument("--label", type=str, default="")
ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "mosaic_bench.json")
opt = ap.parse_args()

dev = torch.device("cuda")
rng = np.random.default_rng(0)
B, size = opt.batch, (512, 512)
flips = [int(v) for v in rng.integers(0, 4, B)]
words, factors = zip(*(jitter_words(list(rng.permutation(4)), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.85, 1.15),
                                    rng.uniform(-0.05, 0.05)) for _ in range(B)))
jitter = (list(words), list(factors))
mosaic = half = full = None
if opt.mosaic == "both":
    from structuredetector_amd.data.augment import mosaic_tiles  # noqa: E402
    W, H = size
    tiles = [mosaic_tiles(size, b, (int(rng.integers(W // 4, 3 * W // 4 + 1)), int(rng.integers(H // 4, 3 * H // 4 + 1)),
                                    tuple(int(v) for v in rng.integers(0, B, 3)))) for b in range(B)]       # every image selected: the policy's draws
    mosaic = ([t[0] for t in tiles], [t[1] for t in tiles])
    half = [t[1][3] for t in tiles]
    full = [[1.0, 0.0, 0.5, 0.0, 1.0, 0.5]] * B


def timed_rounds(fns):
    """us per call of every function in fns, per round: {name: [round 0, round 1, ...]}."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(opt.rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(opt.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per[k].append(e0.elapsed_time(e1) / opt.reps * 1e3)
    return per


def summary(extras):
    med = statistics.median(extras)
    return {"per_round_us": [round(v, 1) for v in extras], "median_us": round(med, 1), "min_us": round(min(extras), 1), "max_us": round(max(extras), 1),
            "spread_over_median": round((max(extras) - min(extras)) / med, 3) if med > 0 else None}


rows, yardstick = [], []
npix = B * size[0] * size[1]
for (H, W) in ((512, 512), (2048, 2448)):
    x = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    table = torch.tensor([x[b].data_ptr() for b in range(B)], dtype=torch.int64, device=dev)
    for form in ("packed", "list"):
        for jit_name, jit in (("off", None), ("on", jitter)):
            def call(**kw):
                if form == "packed":
                    return lambda: preprocess_images(x, size, flips, jitter=jit, **kw)
                return lambda: preprocess_image_list(table, H, W, size, flips, jitter=jit, **kw)
            fns = {"off": call()}
            if mosaic is not None:
                fns["mosaic"] = call(mosaic=mosaic)
                fns["affine_half"] = call(affine=half)
                fns["affine_full"] = call(affine=full)
            per = timed_rounds(fns)
            base = {"source": f"{W}x{H}", "out": "512x512", "batch": B, "form": form, "jitter": jit_name}
            row = dict(base, mosaic="off", us_per_call=round(min(per["off"]), 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
            if mosaic is None:
                continue
            kernel = "k_mosaic_u8" if jit is not None else "k_mosaic_norm"
            moved = npix * (6 if jit is not None else 15)
            row = dict(base, mosaic="on", us_per_call=round(min(per["mosaic"]), 1), extra_us_over_mosaic_off=round(min(per["mosaic"]) - min(per["off"]), 1),
                       added_kernel=kernel, added_kernel_bytes=moved)
            if opt.hbm_tbs > 0:
                row["added_kernel_hbm_floor_us"] = round(moved / (opt.hbm_tbs * 1e12) * 1e6, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            extras = {k: [a - b for a, b in zip(per[k], per["off"])] for k in ("mosaic", "affine_half", "affine_full")}
            y = dict(base, mosaic_kernel=kernel, affine_kernel="k_affine_u8" if jit is not None else "k_affine_norm",
                     **{k: summary(v) for k, v in extras.items()})
            for k in ("affine_half", "affine_full"):
                y[f"mosaic_over_{k}"] = round(y["mosaic"]["median_us"] / y[k]["median_us"], 3) if y[k]["median_us"] > 0 else None
            yardstick.append(y)
            print(json.dumps(y), flush=True)
    del x, table
doc = {"tool": "tools/mosaic_bench.py", "label": opt.label, "device": torch.cuda.get_device_name(0), "reps": opt.reps, "rounds": opt.rounds,
       "hbm_copy_tbs": opt.hbm_tbs or None, "rows": rows, "yardstick": yardstick}
opt.out.parent.mkdir(parents=True, exist_ok=True)
opt.out.write_text(json.dumps(doc, indent=1) + "\n")
