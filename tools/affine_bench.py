#!/usr/bin/env python3
"""GPU time of the preprocess call with and without the random affine warp, bs = 64: 512x512 -> 512x512 and 2448x2048 -> 512x512, jitter on
and off, packed and list forms.  Device events around `--reps` calls, best of `--rounds` rounds, after a warm-up of every shape.  Beside each
row with the warp: the extra time over the same row without it and the HBM floor of the added launch (k_affine_u8: 3 B read + 3 B written
per pixel; k_affine_norm: 3 B read + 12 B written) at `--hbm_tbs` TB/s (what tools/hbm_rw_micro.py reports for a copy on the same box).
`--affine off` times only the rows without the warp: that also runs on a commit that has no warp, for the comparison with the parent.
Writes one JSON document (default profiles/affine_bench.json)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from structuredetector_amd.data import preprocess_image_list, preprocess_images  # noqa: E402
from structuredetector_amd.data.augment import jitter_words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--affine", choices=["both", "off"], default="both")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--hbm_tbs", type=float, default=0.0, help="measured HBM copy rate in TB/s for the floors (0 = leave them out)")
ap.add_argument("--label", type=str, default="")
ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "affine_bench.json")
opt = ap.parse_args()

dev = torch.device("cuda")
rng = np.random.default_rng(0)
B, size = opt.batch, (512, 512)
flips = [int(v) for v in rng.integers(0, 4, B)]
words, factors = zip(*(jitter_words(list(rng.permutation(4)), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.85, 1.15),
                                    rng.uniform(-0.05, 0.05)) for _ in range(B)))
jitter = (list(words), list(factors))
mats = None
if opt.affine == "both":
    from structuredetector_amd.data.augment import affine_inverse_matrix  # noqa: E402
    mats = np.asarray([affine_inverse_matrix(size, rng.uniform(-30, 30), rng.uniform(0.8, 1.2), (rng.uniform(-51.2, 51.2), rng.uniform(-51.2, 51.2)))
                       for _ in range(B)])


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(opt.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(opt.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / opt.reps)
    return best * 1e3                                                           # us per call


rows = []
npix = B * size[0] * size[1]
for (H, W) in ((512, 512), (2048, 2448)):
    x = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    table = torch.tensor([x[b].data_ptr() for b in range(B)], dtype=torch.int64, device=dev)
    for form in ("packed", "list"):
        for jit_name, jit in (("off", None), ("on", jitter)):
            base = None
            for warp in ((None,) if mats is None else (None, mats)):
                kw = {} if warp is None else {"affine": warp}
                if form == "packed":
                    us = timed(lambda: preprocess_images(x, size, flips, jitter=jit, **kw))
                else:
                    us = timed(lambda: preprocess_image_list(table, H, W, size, flips, jitter=jit, **kw))
                row = {"source": f"{W}x{H}", "out": "512x512", "batch": B, "form": form, "jitter": jit_name, "affine": "off" if warp is None else "on",
                       "us_per_call": round(us, 1)}
                if warp is None:
                    base = us
                else:
                    kernel = "k_affine_u8" if jit is not None else "k_affine_norm"
                    moved = npix * (6 if jit is not None else 15)
                    row.update(extra_us_over_affine_off=round(us - base, 1), added_kernel=kernel, added_kernel_bytes=moved)
                    if opt.hbm_tbs > 0:
                        row["added_kernel_hbm_floor_us"] = round(moved / (opt.hbm_tbs * 1e12) * 1e6, 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
    del x, table
doc = {"tool": "tools/affine_bench.py", "label": opt.label, "device": torch.cuda.get_device_name(0), "reps": opt.reps, "rounds": opt.rounds,
       "hbm_copy_tbs": opt.hbm_tbs or None, "rows": rows}
opt.out.parent.mkdir(parents=True, exist_ok=True)
opt.out.write_text(json.dumps(doc, indent=1) + "\n")
