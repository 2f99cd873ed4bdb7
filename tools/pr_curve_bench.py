#!/usr/bin/env python3
"""`evaluate --pr_curve`, measured in one process:

  * device time of `sd_eval_match` at the cfg shape (bs = 64, 128 x 128 maps, 2 + 1 maps, K = 20, P = 40, about 5 objects per image) and
    at the stress shape (bs = 16, 256 x 256 maps, 8 + 8 maps, K = 128, P = 512, 64 - 96 objects), on the lists `sd_decode` wrote for
    heads rendered from the scenes (exact top-k), beside the decoder at the same shape (`Decoder.decode_packed`, the dispatch `evaluate`
    takes) and beside the host time per image of the numpy restatement of the matcher (tests/pr_curve_ref.py), which is what a host-side
    sweep would start from.  Device events around `--launches` back-to-back launches queued behind a stand-in launch (the first timed
    launch does not wait for the host), candidates alternated round by round, median (min - max) over `--rounds` after a warm-up round;
  * wall time per image of `evaluate` over `--n` PNG + JSON samples (tools/feed_bench.write_samples, seeded random-init checkpoint, the
    command of tools/evaluate_bench.py at --eval_batch 16) with and without `--pr_curve`, alternated, median (min - max) over `--repeats`
    after one warm-up pass each.

Random-init weights: this measures time only and says nothing about accuracy.
usage: pr_curve_bench.py [--out profiles/pr_curve_bench.json] [--rounds 7] [--launches 50] [--n 256] [--repeats 5] [--dir /tmp/sd_pr_curve] [--skip_evaluate]"""
import argparse
import contextlib
import io
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def spread(samples, scale=1.0, digits=2):
    return {"median": round(statistics.median(samples) * scale, digits), "min": round(min(samples) * scale, digits),
            "max": round(max(samples) * scale, digits), "n": len(samples)}


def event_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                                                       # the stand-in: the timed launches queue behind it
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def kernel_shape(name, B, M, N, size, K, P, n_min, n_max, rounds, launches):
    from bench import make_args
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import Decoder, Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    from tests import pr_curve_ref as R
    dev = torch.device("cuda")
    args = make_args(dev, M, N, K, P)
    args.width = args.height = size
    args.dist_threshold = 0.05
    rng = np.random.default_rng(B)
    n_obj, o_lab, o_xy, o_np, p_kind, p_xy = synthetic_batch(rng, B, size, size, M, N, n_min=n_min, n_max=n_max)
    enc, dec = Encode(args), Decoder(args)
    tgt = enc.render(enc.plan(size, size, n_obj, o_lab, o_xy, o_np, p_kind, p_xy), dev)
    hm = torch.cat([tgt["anchor_hm"], tgt["part_hm"]], 1).clamp(1e-4, 0.95)
    gen = torch.Generator(device=dev).manual_seed(0)
    head = torch.cat([torch.log(hm / (1 - hm)) + 0.05 * torch.randn(hm.shape, device=dev, generator=gen),
                      0.1 * torch.randn(B, 4, size // 4, size // 4, device=dev, generator=gen)], 1)
    outs = {"anchor_hm": head[:, :M], "part_hm": head[:, M:M + N], "offsets": head[:, M + N:M + N + 2], "embeddings": head[:, M + N + 2:]}
    packed, _ = dec.decode_packed(outs, 0.5, 0.1, exact_topk=True)
    # ground-truth tables straight from the scene arrays: img_size = the input size, so fx = fy = 1
    parts_per_image = np.add.reduceat(o_np, np.concatenate([[0], np.cumsum(n_obj)[:-1]]))
    off = np.concatenate([[0], np.cumsum(n_obj), n_obj.sum() + np.cumsum(parts_per_image)]).astype(np.int32)
    gt_xy = np.concatenate([o_xy, p_xy]).astype(np.float64)
    gt_cls = np.concatenate([o_lab, p_kind]).astype(np.int32)
    img = np.tile(np.asarray([[1.0, 1.0, size * args.dist_threshold]]), (B, 1))
    d_xy, d_cls, d_off, d_img = (torch.from_numpy(v).to(dev) for v in (gt_xy, gt_cls, off, img))
    match = torch.empty((B, K + P), dtype=torch.int32, device=dev)
    dist = torch.empty((B, K + P), dtype=torch.float64, device=dev)
    a_ptr = packed.data_ptr()
    lib, G = L.lib(), len(gt_cls)

    def launch_match():
        L.check(lib.sd_eval_match(a_ptr, a_ptr + 16 * B * K, B, K, P, d_xy.data_ptr(), d_cls.data_ptr(), d_off.data_ptr(), G, d_img.data_ptr(), 4.0, 4.0,
                                  match.data_ptr(), dist.data_ptr(), L.stream()), "sd_eval_match")

    def launch_decode():
        dec.decode_packed(outs, 0.5, 0.1, exact_topk=True)

    samples = {"sd_eval_match": [], "sd_decode": []}
    for r in range(rounds + 1):
        for key, fn in (("sd_eval_match", launch_match), ("sd_decode", launch_decode)):
            t = event_ms(fn, launches)
            if r:
                samples[key].append(t)
    host = dec.split_packed(packed.cpu().numpy(), B, K, P)
    case = dict(a_list=host["anchor_out"], p_list=host["part_out"], gt_xy=gt_xy, gt_cls=gt_cls, gt_off=off, img=img, sx=4.0, sy=4.0)
    want_m, want_d = R.match_ref(case)
    torch.cuda.synchronize()
    got_m, got_d = match.cpu().numpy(), dist.cpu().numpy()
    fin = np.isfinite(want_d)
    agree = bool(np.array_equal(got_m, want_m) and (np.abs(got_d[fin] - want_d[fin]) <= 4 * np.spacing(want_d[fin])).all())
    ref = []
    for _ in range(5):
        t0 = time.perf_counter()
        R.match_ref(case)
        ref.append((time.perf_counter() - t0) / B)
    return {"shape": {"B": B, "maps": [M, N], "map": [size // 4, size // 4], "K": K, "P": P, "objects_per_image": [n_min, n_max], "G": G},
            "sd_eval_match_us_per_launch": spread(samples["sd_eval_match"], 1e3), "sd_decode_us_per_call": spread(samples["sd_decode"], 1e3),
            "sd_eval_match_us_per_image": round(statistics.median(samples["sd_eval_match"]) * 1e3 / B, 3),
            "numpy_reference_host_us_per_image": spread(ref, 1e6, 1), "hits": int((want_m >= 0).sum()), "slots": int(want_m.size),
            "equals_numpy_reference": agree}


def evaluate_wall(n, size, directory, repeats):
    from argparse import Namespace

    from structuredetector_amd.cli import evaluate
    from structuredetector_amd.model import Network
    from tools.feed_bench import write_samples
    root = Path(directory)
    labels = write_samples(root / "valid", n, size)
    ckpt = root / "seeded.pth"
    if not ckpt.exists():
        Network(Namespace(labels={"bean": 0, "maize": 1}, parts={"leaf": 0}, fpn_depth=128), pretrained=False).save(ckpt)
    base = ["--valid_dir", str(root / "valid"), "--labels", str(labels), "-s", "stem", "-W", str(size), "-H", str(size), "-o", str(ckpt)]
    variants = {"without": [], "with_pr_curve": ["--pr_curve"]}
    samples = {k: [] for k in variants}
    for rep in range(repeats + 1):                              # pass 0: page cache warm, kernels loaded
        for key, extra in variants.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                evaluate.main(base + extra)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if rep:
                samples[key].append(dt / n)
    return {"samples": n, "input": [size, size], "eval_batch": 16,
            "ms_per_image": {k: spread(v, 1e3, 3) for k, v in samples.items()},
            "added_ms_per_image_median": round((statistics.median(samples["with_pr_curve"]) - statistics.median(samples["without"])) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pr_curve_bench.json"))
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--n", type=int, default=256); ap.add_argument("--size", type=int, default=512); ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default="/tmp/sd_pr_curve"); ap.add_argument("--skip_evaluate", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pr_curve_bench.py measures on the GPU: no device visible")
    torch.cuda.set_device(0)
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "launches_per_sample": a.launches,
              "cfg": kernel_shape("cfg", 64, 2, 1, 512, 20, 40, 3, 7, a.rounds, a.launches),
              "stress": kernel_shape("stress", 16, 8, 8, 1024, 128, 512, 64, 96, a.rounds, a.launches)}
    if not a.skip_evaluate:
        result["evaluate_wall"] = evaluate_wall(a.n, a.size, a.dir, a.repeats)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
