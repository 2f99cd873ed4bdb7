#!/usr/bin/env python3
"""GPU time of the histogram tone stage (`train --aug_equalize / --aug_autocontrast`), bs = 64, network input 512x512.  Device events
around `--reps` calls, `--rounds` rounds after a warm-up of every variant; us per call, best round, and the spread (min .. max).

1. `sd_tone_u8` in place on (64, 512, 512, 3) bytes, for the tables all-equalize, all-autocontrast (cutoff 1 %) and half-selected (every
   other image a copy row), on three contents: uniform noise, a constant frame (every lane of the histogram kernel meets one bin: its
   contention worst case) and a scene of tests/golden/evaluate16.npz tiled to size; beside
   - a device copy of the same bytes (`copy_` of the image tensor: 3 B/px read + 3 B/px written), timed in the same process, and
   - its HBM floor of 9 B/px -- the image read for the histogram, read again and written by the look-up -- at the copy rate of a 1 GiB
     fp32 `copy_` (read + write; the measurement of `tools/hbm_rw_micro.py`), taken here in the same process.
   The two launches are timed apart by `rocprofv3 --kernel-trace --stats` over `--stage_only` (a run of its own:
   profiles/tone_kernel_stats.csv); with `--stage_only CONTENT:TABLE` this tool runs that one variant `--reps` times and writes nothing.
2. The training chain (ColorJitter + flips, packed and pointer-list, 2448x2048 sources) with the table that `--aug_equalize 0.25
   --aug_autocontrast 0.5` draws beside the same chain without the flags, which is the previous path (a null table never reaches the new
   code) and is timed before and after: its own run-to-run spread is what a difference has to exceed.

Writes one JSON document (default profiles/tone_bench.json)."""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--label", type=str, default="")
ap.add_argument("--stage_only", type=str, default="", metavar="CONTENT:TABLE", help="run one variant of part 1 and stop (for a kernel trace)")
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "tone_bench.json")
opt = ap.parse_args()

sys.path.insert(0, str(ROOT))
from structuredetector_amd import _lib as L  # noqa: E402
from structuredetector_amd.data import preprocess_image_list, preprocess_images, tone_images, tone_rows  # noqa: E402
from structuredetector_amd.data.augment import TONE_AUTOCONTRAST, TONE_COPY, TONE_EQUALIZE, jitter_words  # noqa: E402

dev = torch.device("cuda")
rng = np.random.default_rng(0)
B, size, (H, W) = opt.batch, (512, 512), (2048, 2448)
P_EQ, P_AC, CUTOFF = 0.25, 0.5, 1.0
n_pixels = size[0] * size[1]


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


def golden_scene():
    """One scene of tests/golden/evaluate16.npz as the suite materialises it, tiled to the network input."""
    from PIL import Image
    from tests.helpers import write_evaluate16_dir
    with tempfile.TemporaryDirectory() as tmp:
        write_evaluate16_dir(np.load(ROOT / "tests" / "golden" / "evaluate16.npz"), tmp)
        a = np.asarray(Image.open(Path(tmp) / "img_00.png").convert("RGB"))
    reps = (-(-size[1] // a.shape[0]), -(-size[0] // a.shape[1]), 1)
    return np.tile(a, reps)[:size[1], :size[0]].copy()


def content(kind):
    if kind == "noise":
        return torch.from_numpy(rng.integers(0, 256, (B, size[1], size[0], 3), dtype=np.uint8)).to(dev)
    if kind == "constant":
        return torch.from_numpy(np.broadcast_to(np.asarray([124, 116, 104], dtype=np.uint8), (B, size[1], size[0], 3)).copy()).to(dev)
    return torch.from_numpy(np.broadcast_to(golden_scene(), (B, size[1], size[0], 3)).copy()).to(dev)


TABLES = {"equalize": [(TONE_EQUALIZE, 0.0)] * B, "autocontrast": [(TONE_AUTOCONTRAST, CUTOFF)] * B,
          "half": [(TONE_EQUALIZE, 0.0) if i % 4 == 0 else (TONE_AUTOCONTRAST, CUTOFF) if i % 4 == 2 else (TONE_COPY, 0.0) for i in range(B)]}
lib = L.lib()
ws = L.workspace(lib.sd_tone_workspace_bytes(B), dev)


def stage_call(img, rows_dev):
    """The memset and the two launches alone, in place (the chain's use): the table is on the device already."""
    return lambda: L.check(lib.sd_tone_u8(img.data_ptr(), img.data_ptr(), B, size[1], size[0], rows_dev.data_ptr(), ws.data_ptr(), ws.numel(),
                                          L.stream()), "sd_tone_u8")


if opt.stage_only:
    kind, name = opt.stage_only.split(":")
    src = content(kind)
    img = src.clone()
    rows_dev = torch.tensor(tone_rows(TABLES[name], n_pixels), dtype=torch.int32, device=dev)
    call = stage_call(img, rows_dev)
    for _ in range(opt.reps):
        img.copy_(src)                                                          # in place changes the content: every call sees the source
        call()
    torch.cuda.synchronize()
    sys.exit(0)

doc = {"tool": "tools/tone_bench.py", "label": opt.label, "device": torch.cuda.get_device_name(0), "reps": opt.reps, "rounds": opt.rounds,
       "batch": B, "out": "512x512"}

a = torch.empty(1 << 28, device=dev)
b = torch.empty(1 << 28, device=dev)
best, worst = timed(lambda: b.copy_(a), reps=5)
copy_tbs = 2 * (1 << 30) / 1e12 / (best * 1e-6)
doc["hbm_copy"] = {"what": "1 GiB fp32 copy_ (read + write), the measurement of tools/hbm_rw_micro.py", "us": round(best, 1), "tb_per_s": round(copy_tbs, 3)}
print(json.dumps(doc["hbm_copy"]), flush=True)
del a, b

doc["stage"] = []
for kind in ("noise", "constant", "golden"):
    src = content(kind)
    img = src.clone()
    copy_best, copy_worst = timed(lambda: img.copy_(src), reps=50)
    for name, draws in TABLES.items():
        table = tone_rows(draws, n_pixels)
        rows_dev = torch.tensor(table, dtype=torch.int32, device=dev)
        assert torch.equal(tone_images(src, table), tone_images(src, table))
        call = stage_call(img, rows_dev)

        def both():
            img.copy_(src)                                                      # the stage runs in place: restore the content, then subtract the copy
            call()
        best, worst = timed(both, reps=50)
        best, worst = best - copy_best, worst - copy_best
        selected = sum(m != TONE_COPY for m, _ in draws)
        floor_bytes = 9 * n_pixels * selected                                   # a copy row in place costs nothing
        floor_us = floor_bytes / (copy_tbs * 1e12) * 1e6
        row = {"entry": "sd_tone_u8 (in place)", "content": kind, "table": name, "selected": selected, "us_per_call": round(best, 1),
               "spread_us": [round(best, 1), round(worst, 1)], "image_copy_us": round(copy_best, 1),
               "times_the_image_copy": round(best / copy_best, 2), "hbm_floor_bytes": floor_bytes, "hbm_floor_us_at_copy_rate": round(floor_us, 1),
               "reached_fraction_of_floor": round(floor_us / best, 3), "tb_per_s": round(floor_bytes / 1e12 / (best * 1e-6), 3)}
        doc["stage"].append(row)
        print(json.dumps(row), flush=True)
    del src, img

flips = [int(v) for v in rng.integers(0, 4, B)]
words, factors = zip(*(jitter_words(list(rng.permutation(4)), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.85, 1.15),
                                    rng.uniform(-0.05, 0.05)) for _ in range(B)))
jitter = (list(words), list(factors))
u = rng.uniform(0, 1, (B, 3))
draws = [(TONE_EQUALIZE, 0.0) if u0 < P_EQ else (TONE_AUTOCONTRAST, CUTOFF * u2) if u1 < P_AC else (TONE_COPY, 0.0) for u0, u1, u2 in u]
tone = tone_rows(draws, n_pixels)
doc["chain_tone_table"] = {"aug_equalize": P_EQ, "aug_autocontrast": P_AC, "aug_autocontrast_cutoff": CUTOFF,
                           "equalized": sum(m == TONE_EQUALIZE for m, _ in draws), "autocontrasted": sum(m == TONE_AUTOCONTRAST for m, _ in draws)}

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
    on_best, on_worst = timed(lambda: call(tone=tone))
    again_best, again_worst = timed(call)                                       # the flag-off call once more: its run-to-run spread
    off_best, off_worst = min(off_best, again_best), max(off_worst, again_worst)
    row = {"source": f"{W}x{H}", "form": form, "chain": "jitter_flips", "tone_us_per_call": round(on_best, 1),
           "tone_spread_us": [round(on_best, 1), round(on_worst, 1)], "tone_minus_off_us": round(on_best - off_best, 1),
           "off_us_per_call": round(off_best, 1), "off_spread_us": [round(off_best, 1), round(off_worst, 1)]}
    rows.append(row)
    print(json.dumps(row), flush=True)
doc["chain"] = rows
opt.out.parent.mkdir(parents=True, exist_ok=True)
opt.out.write_text(json.dumps(doc, indent=1) + "\n")
