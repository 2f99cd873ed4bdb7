#!/usr/bin/env python3
"""`train --train_dir` throughput with the device-resident image cache (`--cache_images`, data/image_cache.py) next to the host feed and
the synthetic-tensor step, on two locally generated sets: 512 x 512 PNG (tools/feed_bench.py's samples) and 2448 x 2048 JPEG (the
reference dataset's camera frames, reference README "Annotation").  Per set and precision: the host-path rate (what every epoch costs
without the cache), the prefill time and the cached rate (epoch >= 2; epoch 1 = prefill + one cached epoch), hit rate, the host
breakdown of a cached step (wait / augment / encode / step) and the peak device memory with the cache.
`--kernel_ab` instead times the horizontal pass alone: the packed path (k_resample_h) against the pointer-table path
(k_resample_h_list) on a batch of 2448 x 2048 sources -> 512 x 512 (run it under `rocprofv3 --kernel-trace --stats` for per-kernel times).
usage: feed_cache_bench.py [--sets png512,jpeg2448] [--n_png 512] [--n_jpeg 256] [--batch 64] [--steps 24] [--amp] [--dir /tmp/sd_feed_cache]
       feed_cache_bench.py --kernel_ab [--batch 64] [--iters 20]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))


def write_jpeg_samples(directory, n, width=2448, height=2048, seed=7):
    """camera-sized JPEG frames (smooth field + fine noise, quality 90) + JSON scenes from the product's seeded generator"""
    from PIL import Image

    from structuredetector_amd.data.synthetic import synthetic_batch
    directory.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    labels, parts = ["bean", "maize"], ["leaf"]
    for i in range(n):
        low = rng.integers(0, 256, (height // 64, width // 64, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(low).resize((width, height), Image.BICUBIC), np.int16) + rng.integers(-8, 9, (height, width, 3), dtype=np.int16)
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(directory / f"img_{i:04d}.jpg", quality=90)
        n_obj, o_lab, o_xy, o_np, p_kind, p_xy = synthetic_batch(rng, 1, width, height, len(labels), len(parts))
        objs, j = [], 0
        for k in range(int(n_obj[0])):
            ps = [{"kind": parts[int(p_kind[j + q])], "location": {"x": float(p_xy[j + q][0]), "y": float(p_xy[j + q][1])}} for q in range(int(o_np[k]))]
            j += int(o_np[k])
            objs.append({"label": labels[int(o_lab[k])], "box": None,
                         "parts": [{"kind": "stem", "location": {"x": float(o_xy[k][0]), "y": float(o_xy[k][1])}}] + ps})
        js = {"image_path": str(directory / f"img_{i:04d}.jpg"), "img_size": [width, height], "objects": objs}
        (directory / f"img_{i:04d}.json").write_text(json.dumps(js))
    (directory.parent / "feed_labels.json").write_text(json.dumps({"labels": labels, "parts": parts}))
    return directory.parent / "feed_labels.json"


def make_set(root, name, n):
    from feed_bench import write_samples
    d = root / name / "train"
    suffix = ".png" if name == "png512" else ".jpg"
    if len(list(d.glob("*" + suffix))) == n and (root / name / "feed_labels.json").exists():
        return d, root / name / "feed_labels.json"
    return d, (write_samples(d, n, 512) if name == "png512" else write_jpeg_samples(d, n))


def run_set(root, name, n, batch, steps, amp, workers):
    from structuredetector_amd.data.feeder import BatchFeeder
    from structuredetector_amd.model.trainer import Trainer, shard_indices
    from structuredetector_amd.utils.args import Arguments
    t0 = time.perf_counter()
    d, labels = make_set(root, name, n)
    out = {"set": name, "samples": n, "mb_per_file": round(sum(f.stat().st_size for f in d.glob("img_*.[pj][np]g")) / n / 1e6, 3),
           "write_s": round(time.perf_counter() - t0, 1), "batch": batch, "amp": amp}
    common = ["--labels", str(labels), "-s", "stem", "-b", str(batch), "-W", "512", "-H", "512", "-e", "1000"] + (["--amp"] if amp else [])
    if workers:
        common += ["--decode_workers", str(workers)]

    def rate(tr, label, warm=4):
        it, k, t_start = tr.batches(), 0, None
        while k < warm + steps:
            try:
                images, targets = next(it)
            except StopIteration:
                tr.epoch += 1
                it = tr.batches()
                continue
            tr.step(images, targets)
            k += 1
            if k == warm:
                torch.cuda.synchronize(); t_start = time.perf_counter()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t_start
        it.close()
        out[label] = round(steps * batch / dt, 1)
        return steps * batch / dt

    threads = torch.get_num_threads()
    try:
        syn = rate(Trainer(Arguments().parse(common + ["--synthetic", str(batch * 8)])), "synthetic_img_s")
        host = rate(Trainer(Arguments().parse(common + ["--train_dir", str(d)])), "host_path_img_s")
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        gb = n * 2448 * 2048 * 3 / 1e9 * 1.05 + 0.1 if name != "png512" else n * 512 * 512 * 3 / 1e9 * 1.05 + 0.1
        tr = Trainer(Arguments().parse(common + ["--train_dir", str(d), "--cache_images", f"{gb:.3f}"]))
        tr.prefill_cache()
        st0 = tr.cache.stats()
        cached = rate(tr, "cached_img_s")
        st = tr.cache.stats()
        epoch_s = n // batch * batch / cached
        out.update(prefill_s=st0["prefill_seconds"], cache_gb=round(st0["bytes_used"] / 1e9, 3), refused=st0["refused"],
                   epoch1_img_s=round(n / (st0["prefill_seconds"] + epoch_s), 1), epoch2_img_s=out["cached_img_s"],
                   hit_rate=round(st["hits"] / max(st["hits"] + st["misses"], 1), 4),
                   host_over_synthetic=round(host / syn, 3), cached_over_synthetic=round(cached / syn, 3))
        # host breakdown of cached steps: waiting for the feeder, augmentation call, target encoding, step launch
        shards = shard_indices(len(tr.dataset), batch, 0, 1, 1)
        feed = iter(BatchFeeder(tr.dataset, shards * 8, tr.args.device, depth=3, cache=tr.cache))
        acc = {"wait": 0.0, "augment": 0.0, "encode": 0.0, "step": 0.0}
        torch.set_num_threads(1)
        for i in range(4 + 12):
            t0 = time.perf_counter(); b = next(feed)
            t1 = time.perf_counter(); images, anns = tr.augment(b, b.annotations)
            t2 = time.perf_counter(); targets = tr.encode.batch(tr.augment.size, anns, tr.args.device)
            t3 = time.perf_counter(); tr.step(images, targets)
            t4 = time.perf_counter()
            if i >= 4:
                for key, v in zip(acc, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    acc[key] += v / 12 * 1e3
        torch.cuda.synchronize()
        feed.close()
        out["cached_host_ms_per_step"] = {key: round(v, 2) for key, v in acc.items()}
        out["synthetic_ms_per_step"] = round(batch / syn * 1e3, 2)
        out["peak_gb_with_cache"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        del tr
        torch.cuda.empty_cache()
    finally:
        torch.set_num_threads(threads)
    return out


def kernel_ab(batch, iters, hin=2048, win=2448, size=(512, 512)):
    """The whole preprocess call (horizontal + vertical/normalise) on the packed tensor and through the pointer table, same bytes; the
    horizontal passes alone come from a kernel trace.  Source bytes per call: batch * hin * win * 3."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(0)
    packed = torch.randint(0, 256, (batch, hin, win, 3), dtype=torch.uint8, device=dev, generator=g)
    table = torch.tensor([packed[b].data_ptr() for b in range(batch)], dtype=torch.int64, device=dev)
    assert torch.equal(preprocess_images(packed, size), preprocess_image_list(table, hin, win, size))
    out = {"batch": batch, "source": [hin, win], "out": list(size), "source_gb": round(batch * hin * win * 3 / 1e9, 3)}
    for label, fn in (("packed_ms", lambda: preprocess_images(packed, size)), ("list_ms", lambda: preprocess_image_list(table, hin, win, size))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[label] = round(e0.elapsed_time(e1) / iters, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="png512,jpeg2448"); ap.add_argument("--n_png", type=int, default=512); ap.add_argument("--n_jpeg", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64); ap.add_argument("--steps", type=int, default=24); ap.add_argument("--workers", type=int, default=0)
    ap.add_argument("--amp", action="store_true"); ap.add_argument("--dir", default="/tmp/sd_feed_cache")
    ap.add_argument("--kernel_ab", action="store_true"); ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.kernel_ab:
        print(json.dumps(kernel_ab(a.batch, a.iters)), flush=True)
        return
    for name in a.sets.split(","):
        print(json.dumps(run_set(Path(a.dir), name, a.n_png if name == "png512" else a.n_jpeg, a.batch, a.steps, a.amp, a.workers)), flush=True)


if __name__ == "__main__":
    main()
