#!/usr/bin/env python3
"""Validation wall time per image at world 1: `Trainer.valid()` (one Encode + one `Loss.per_image` launch pair per batch) against the
per-image loss path it replaced (one Encode.batch + one Loss call per image on that image's slice of the batched head), on a directory
of `--copies` x the 16 evaluate16 samples (tests/helpers.py:write_evaluate16_dir; 512 images by default).  Both passes share everything
else: the batched feed, forward and decoder, and the Evaluator.  Checks that both give the same loss bits, then prints one JSON line.
usage: valid_bench.py [--copies 32] [--eval_batch 16] [--reps 3] [--dir /tmp/sd_valid_bench]"""
import argparse
import json
import shutil
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def write_set(directory, copies):
    from tests.helpers import write_evaluate16_dir
    g = np.load(ROOT / "tests" / "golden" / "evaluate16.npz")
    src = directory / "src"
    write_evaluate16_dir(g, src)
    out = directory / "valid"
    out.mkdir(parents=True, exist_ok=True)
    for c in range(copies):
        for n in range(16):
            name = f"img_{c:03d}_{n:02d}"
            shutil.copyfile(src / f"img_{n:02d}.png", out / f"{name}.png")
            js = json.loads((src / f"img_{n:02d}.json").read_text())
            js["image_path"] = str(out / f"{name}.png")
            (out / f"{name}.json").write_text(json.dumps(js))
    (directory / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    return out


def per_image_pass(tr):
    """The loop of the parent's Trainer.valid(): evaluator + one Encode.batch + one Loss call per image."""
    from structuredetector_amd.model.loss import LossStats
    from structuredetector_amd.model.predictor import batched_outputs
    a = tr.args
    tr.net.eval()
    tr.evaluator.reset()
    per_image = []
    for prediction, annotation, raw_parts, output in batched_outputs(tr.net, tr.decoder, tr.valid_set, a, keep_output=True):
        with torch.no_grad():
            tr.evaluator.accumulate(prediction, annotation, raw_parts, eval_csi=True, eval_classif=True)
            target = tr.encode.batch((a.width, a.height), [annotation], a.device)
            tr.loss(output, target)
        per_image.append(torch.stack([tr.loss.stats.hm_loss, tr.loss.stats.offset_loss, tr.loss.stats.embedding_loss]))
    stats = LossStats(*(torch.stack(per_image).double().sum(0).tolist()))
    tr.net.train()
    stats /= len(per_image)
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=32)
    ap.add_argument("--eval_batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/sd_valid_bench")
    o = ap.parse_args()
    from structuredetector_amd.model.trainer import Trainer
    from structuredetector_amd.utils.args import Arguments
    directory = Path(o.dir)
    valid = write_set(directory, o.copies)
    args = Arguments().parse(["--train_dir", str(valid), "--valid_dir", str(valid), "-s", "stem", "--labels", str(directory / "labels.json"),
                              "--eval_batch", str(o.eval_batch), "--log_dir", str(directory / "log")])
    torch.manual_seed(0)
    tr = Trainer(args)
    tr.save_dir = directory / "run"

    def batched():
        tr.best_loss, tr.best_csi, tr.best_classif, tr.best_kp_reg = float("-inf"), 2.0, 2.0, 2.0     # no checkpoint writes in the timing
        return tr.valid()

    times = {"per_image": [], "batched": []}
    results = {}
    for name, fn in (("per_image", lambda: per_image_pass(tr)), ("batched", batched)) * (o.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = fn()
        torch.cuda.synchronize()
        times[name].append(time.perf_counter() - t0)
        results[name] = (stats.hm_loss, stats.offset_loss, stats.embedding_loss)
    assert results["per_image"] == results["batched"], results
    n = len(tr.valid_set)
    rec = {"images": n, "eval_batch": o.eval_batch, "reps": o.reps, "same_bits": True}
    for name, ts in times.items():
        ts = sorted(ts[1:])                                                   # first pass of each: warm-up
        rec[f"{name}_ms_per_image_median"] = round(ts[len(ts) // 2] / n * 1e3, 4)
        rec[f"{name}_s_all"] = [round(t, 3) for t in times[name]]
    rec["ratio_batched_over_per_image"] = round(rec["batched_ms_per_image_median"] / rec["per_image_ms_per_image_median"], 4)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
