#!/usr/bin/env python3
"""GPU time of the windowed resize of `train --train_tiles` next to the whole-frame resize the training step pays without it, bs = 64 from
2448x2048 sources in one device arena (odd byte offsets, as a decoded-image cache holds them): grid 3x3, 512x512 windows, overlap 64, so a
1408x1408 canvas and origins uniform over it (seeded).  Per form -- plain (window / resize + Normalize) and jitter + flips -- three variants:
  whole_frame_list   preprocess_image_list(sources -> 512x512): what the step runs today, unchanged by the feature
  window_list        the same call with window=(canvas, origins): sd_preprocess_images_list_window
  window_packed      preprocess_images with the window on the same images packed in one tensor: sd_preprocess_images_window
Device events around `--reps` calls, `--rounds` rounds after a warm-up of every variant; within a round the variants run one after the other,
so a round's ratios see the same machine state.  Beside each window row: the bytes the pass has to move -- the source bytes under each
window read once (from the host's copy of the tables, per origin), the 8-bit intermediate written once and read once, for jitter + flips
the 8-bit window written once and read twice (grey sums, jitter), the fp32 output written once -- and the time those bytes take at the
HBM copy rate (`--hbm_tbs` TB/s, or a 1 GB device-to-device copy timed in this process).  Writes one JSON document (default
profiles/train_tiles_bench.json)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from structuredetector_amd.data import preprocess_image_list, preprocess_images, window_extents  # noqa: E402
from structuredetector_amd.data.augment import jitter_words, pil_bilinear_coeffs  # noqa: E402
from structuredetector_amd.utils.args import tile_canvas  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--source", type=str, default="2448x2048", help="WIDTHxHEIGHT of the source frames")
ap.add_argument("--size", type=int, default=512, help="side of the square window = the network input")
ap.add_argument("--grid", type=int, default=3, help="tiles per axis")
ap.add_argument("--overlap", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--hbm_tbs", type=float, default=0.0, help="HBM copy rate in TB/s for the floors (0 = time a 1 GB copy here)")
ap.add_argument("--label", type=str, default="")
ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "train_tiles_bench.json")
opt = ap.parse_args()

dev = torch.device("cuda")
rng = np.random.default_rng(0)
B, size = opt.batch, (opt.size, opt.size)
Win, Hin = (int(v) for v in opt.source.lower().split("x"))
canvas = tile_canvas(opt.size, opt.size, (opt.grid, opt.grid), opt.overlap)
origins = [(int(rng.integers(0, canvas[0] - size[0] + 1)), int(rng.integers(0, canvas[1] - size[1] + 1))) for _ in range(B)]
flips = [int(v) for v in rng.integers(0, 4, B)]
words, factors = zip(*(jitter_words(list(rng.permutation(4)), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.85, 1.15),
                                    rng.uniform(-0.05, 0.05)) for _ in range(B)))
jitter = (list(words), list(factors))

# the sources: one packed tensor, and the same bytes in an arena at odd offsets behind a pointer table
gen = torch.Generator(device=dev).manual_seed(0)
packed = torch.randint(0, 256, (B, Hin, Win, 3), dtype=torch.uint8, device=dev, generator=gen)
nbytes = Hin * Win * 3
offsets = [k * (nbytes + 17) + 1 for k in range(B)]
arena = torch.empty(offsets[-1] + nbytes + 64, dtype=torch.uint8, device=dev)
for k, off in enumerate(offsets):
    arena[off:off + nbytes].copy_(packed[k].reshape(-1))
table = torch.tensor([arena.data_ptr() + off for off in offsets], dtype=torch.int64, device=dev)


def span(bounds, o, n):
    return int(bounds[o + n - 1, 0] + bounds[o + n - 1, 1] - bounds[o, 0])


hb, vb = pil_bilinear_coeffs(Win, canvas[0])[0], pil_bilinear_coeffs(Hin, canvas[1])[0]
spans = [(span(hb, x0, size[0]), span(vb, y0, size[1])) for x0, y0 in origins]          # (columns, rows) under each window
max_cols, max_rows = window_extents(Win, canvas[0], size[0]), window_extents(Hin, canvas[1], size[1])
npix = B * size[0] * size[1]
source_bytes = sum(c * r * 3 for c, r in spans)
inter_bytes = sum(r * size[0] * 3 for _, r in spans)
moved = {"plain": source_bytes + 2 * inter_bytes + npix * 12, "jitter_flips": source_bytes + 2 * inter_bytes + npix * 3 * 3 + npix * 12}
whole_moved = {"plain": B * nbytes + 2 * B * Hin * size[0] * 3 + npix * 12, "jitter_flips": B * nbytes + 2 * B * Hin * size[0] * 3 + npix * 3 * 3 + npix * 12}


def copy_rate():
    """TB/s of a 1 GB device-to-device copy (bytes read + bytes written over the time), best of 5 timed windows of 10 copies."""
    src, dst = torch.empty(1 << 30, dtype=torch.uint8, device=dev), torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    for _ in range(3):
        dst.copy_(src)
    best = float("inf")
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 10 * 1e-3)
    return 2 * (1 << 30) / best / 1e12


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


def summary(us):
    med = statistics.median(us)
    return {"per_round_us": [round(v, 1) for v in us], "median_us": round(med, 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1),
            "spread_over_median": round((max(us) - min(us)) / med, 3)}


tbs = opt.hbm_tbs or copy_rate()
rows = []
for form, kw in (("plain", {}), ("jitter_flips", dict(flips=flips, jitter=jitter))):
    fns = {"whole_frame_list": lambda kw=kw: preprocess_image_list(table, Hin, Win, size, **kw),
           "window_list": lambda kw=kw: preprocess_image_list(table, Hin, Win, size, window=(canvas, origins), **kw),
           "window_packed": lambda kw=kw: preprocess_images(packed, size, window=(canvas, origins), **kw)}
    same = torch.equal(fns["window_list"](), fns["window_packed"]())            # the two forms compute the same bytes at the timed size
    per = timed_rounds(fns)
    for name, us in per.items():
        nb = whole_moved[form] if name == "whole_frame_list" else moved[form]
        floor = nb / (tbs * 1e12) * 1e6
        row = {"variant": name, "form": form, "batch": B, "source": f"{Win}x{Hin}", "out": f"{size[0]}x{size[1]}", **summary(us),
               "bytes_moved": nb, "hbm_floor_us": round(floor, 1), "floor_over_median": round(floor / statistics.median(us), 3)}
        if name != "whole_frame_list":
            row["canvas"] = f"{canvas[0]}x{canvas[1]}"
            row["per_round_ratio_to_whole_frame"] = [round(a / b, 3) for a, b in zip(us, per["whole_frame_list"])]
            row["list_equals_packed"] = bool(same)
        rows.append(row)
        print(json.dumps(row), flush=True)
doc = {"tool": "tools/train_tiles_bench.py", "label": opt.label, "device": torch.cuda.get_device_name(0), "reps": opt.reps, "rounds": opt.rounds,
       "hbm_copy_tbs": round(tbs, 3), "hbm_copy_tbs_source": "--hbm_tbs" if opt.hbm_tbs else "1 GB device-to-device copy timed in this process",
       "grid": f"{opt.grid}x{opt.grid}", "overlap": opt.overlap, "max_cols": max_cols, "max_rows": max_rows,
       "window_source_bytes_per_image": round(source_bytes / B), "frame_bytes_per_image": nbytes, "rows": rows}
opt.out.parent.mkdir(parents=True, exist_ok=True)
opt.out.write_text(json.dumps(doc, indent=1) + "\n")
