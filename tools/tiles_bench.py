#!/usr/bin/env python3
"""Tiled inference, measured in one process with 128 x 128 tile maps (512 x 512 network input), an overlap of 16 cells (64 px), B = 16
images and the default label set, for the grids 2 x 2 and 3 x 2:

  * `sd_tile_merge_nms` on the heatmap + regression planes of a (T*16, 7 + 4, 128, 128) head tensor (channel-slice views, as `TiledNet`
    passes them), against its HBM floor -- every source plane read once, the canvas planes written once;
  * `sd_nms5` with the sigmoid fused over the same number of source cells (the T*16 heatmap planes), the yardstick beside it;
  * `sd_tile_views` from the (16, 3, Hc, Wc) canvas, against its floor (canvas read once, tiles written once);
  * the floors are taken at the COPY RATE measured in this process (`Tensor.copy_` of 256 MiB, read + write), not at a nominal figure;
  * `evaluate`-style wall time per image from 2448 x 2048 uint8 sources (preprocess + forward + decode submitted one batch ahead of the
    host assembly, as model/predictor.py does): the plain step at 512 x 512, the tiled step, and the plain network run directly at
    `-W Wc -H Hc`, in fp32 and `--bf16_inference`.

Kernel times: device events around `--launches` back-to-back launches, the candidates alternated round by round, median over `--rounds`
after a warm-up round.  Wall times: host clock around `--batches` batches ending in a device synchronise, candidates alternated, median.
Random-init weights: this measures time only and says nothing about accuracy.
usage: tiles_bench.py [--out profiles/tiles_bench.json] [--rounds 7] [--launches 50] [--batches 4]"""
import argparse
import json
import statistics
import sys
import time
from argparse import Namespace
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

GRIDS = ((2, 2), (3, 2))             # (Tx, Ty)


def event_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def alternate(candidates, rounds, measure):
    """{name: median over rounds}: every round measures every candidate once, in turn; round 0 is the warm-up."""
    samples = {name: [] for name in candidates}
    for r in range(rounds + 1):
        for name, fn in candidates.items():
            t = measure(fn)
            if r:
                samples[name].append(t)
    return {name: statistics.median(v) for name, v in samples.items()}, samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tiles_bench.json"))
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--launches", type=int, default=50); ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--skip_steps", action="store_true", help="kernels only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiles_bench.py measures on the GPU: no device visible")
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import Decoder, preprocess_images
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.tiles import TiledNet, tile_views, tiled_decoder
    from structuredetector_amd.utils.args import tile_canvas
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = L.lib()
    names = json.loads((ROOT / "labels.json").read_text())
    labels, parts = {n: i for i, n in enumerate(names["labels"])}, {n: i for i, n in enumerate(names["parts"])}
    M, N = len(labels), len(parts)
    B, h, w, o, nb, R = 16, 128, 128, 16, M + N, 4
    W, H, O = 4 * w, 4 * h, 4 * o
    result = {"device": torch.cuda.get_device_name(dev), "batch": B, "tile_map": [h, w], "overlap_cells": o, "heatmap_channels": nb,
              "regression_channels": R, "rounds": a.rounds, "launches_per_sample": a.launches}

    # ---- the copy rate of this device, in this process: what "read once + write once" costs
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    med, _ = alternate({"copy": lambda: dst.copy_(src)}, a.rounds, lambda fn: event_ms(fn, 10))
    copy_gbs = 2 * src.numel() / med["copy"] / 1e6
    result["copy_rate_gbs_measured"] = round(copy_gbs, 1)
    del src, dst

    gen = torch.Generator(dev).manual_seed(0)
    result["kernels"] = {}
    for tx, ty in GRIDS:
        T = tx * ty
        hc, wc = ty * h - (ty - 1) * o, tx * w - (tx - 1) * o
        head = torch.randn(T * B, nb + R, h, w, device=dev, generator=gen) * 4
        _, p, sb, sc = L.map_view(head[:, :nb])
        _, rp, r_sb, r_sc = L.map_view(head[:, nb:])
        assert p == head.data_ptr()
        out_hm, out_reg = torch.empty(B, nb, hc, wc, device=dev), torch.empty(B, R, hc, wc, device=dev)
        out_nms = torch.empty(T * B, nb, h, w, device=dev)
        Wc, Hc = tile_canvas(W, H, (tx, ty), O)
        canvas = torch.randn(B, 3, Hc, Wc, device=dev, generator=gen)
        kernels = {
            "sd_tile_merge_nms": lambda: L.check(lib.sd_tile_merge_nms(p, sb, sc, nb, rp, r_sb, r_sc, R, out_hm.data_ptr(), out_reg.data_ptr(),
                                                                       B, h, w, ty, tx, o, L.stream()), "sd_tile_merge_nms"),
            "sd_tile_merge_nms heatmaps only": lambda: L.check(lib.sd_tile_merge_nms(p, sb, sc, nb, None, 0, 0, 0, out_hm.data_ptr(), None,
                                                                                     B, h, w, ty, tx, o, L.stream()), "sd_tile_merge_nms"),
            "sd_nms5 sigmoid fused, same source cells": lambda: L.check(lib.sd_nms5(p, sb, sc, out_nms.data_ptr(), T * B, nb, h, w, 1, L.stream()),
                                                                        "sd_nms5"),
            "sd_tile_views": lambda: tile_views(canvas, (tx, ty), O)}
        moved = {"sd_tile_merge_nms": 4 * (T * B * (nb + R) * h * w + B * (nb + R) * hc * wc),
                 "sd_tile_merge_nms heatmaps only": 4 * (T * B * nb * h * w + B * nb * hc * wc),
                 "sd_nms5 sigmoid fused, same source cells": 4 * 2 * T * B * nb * h * w,
                 "sd_tile_views": 4 * 3 * B * (Hc * Wc + T * H * W)}
        med, samples = alternate(kernels, a.rounds, lambda fn: event_ms(fn, a.launches))
        result["kernels"][f"{tx}x{ty}"] = {
            name: {"us": round(ms * 1e3, 2), "min_us": round(min(samples[name]) * 1e3, 2), "max_us": round(max(samples[name]) * 1e3, 2),
                   "bytes": moved[name], "floor_us_at_copy_rate": round(moved[name] / copy_gbs / 1e3, 2),
                   "x_floor": round(ms * 1e3 / (moved[name] / copy_gbs / 1e3), 2), "achieved_gbs": round(moved[name] / ms / 1e6, 1)}
            for name, ms in med.items()}
        del head, out_hm, out_reg, out_nms, canvas
    print(json.dumps({"copy_rate_gbs_measured": result["copy_rate_gbs_measured"], "kernels": result["kernels"]}, indent=1), flush=True)

    # ---- the whole step, per image, from camera-sized sources
    result["step"] = {}
    sources = torch.randint(0, 256, (B, 2048, 2448, 3), dtype=torch.uint8, device=dev, generator=gen)
    for precision, bf16 in (() if a.skip_steps else (("fp32", False), ("bf16_inference", True))):
        def make_args(width, height):
            return Namespace(labels=labels, parts=parts, _r_labels={v: k for k, v in labels.items()}, _r_parts={v: k for k, v in parts.items()},
                             anchor_name="stem", down_ratio=4.0, max_objects=20, max_parts=40, conf_threshold=0.5, decoder_dist_thresh=0.1,
                             fpn_depth=128, bf16_inference=bf16, device=dev, width=width, height=height)
        args = make_args(W, H)
        torch.manual_seed(0)
        net = Network(args, pretrained=False).to(dev).eval()
        plain_dec = Decoder(args)

        def plain(size, decoder):
            return lambda: decoder.submit(net(preprocess_images(sources, size)), with_raw_parts=True)

        def tiled(grid):
            model, decoder = TiledNet(net, args, grid, O), tiled_decoder(args, grid, O)
            return lambda: decoder.submit(model(preprocess_images(sources, (W, H)), at_size=lambda size: preprocess_images(sources, size)),
                                          with_raw_parts=True)
        setups = {f"plain {W}x{H}": plain((W, H), plain_dec)}
        for grid in GRIDS:
            size = tile_canvas(W, H, grid, O)
            setups[f"tiles {grid[0]}x{grid[1]} (canvas {size[0]}x{size[1]})"] = tiled(grid)
            setups[f"plain {size[0]}x{size[1]}"] = plain(size, Decoder(make_args(*size)))

        def loop(step):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pending = None
            with torch.no_grad():
                for _ in range(a.batches):
                    handle = step()
                    if pending is not None:
                        pending.result()
                    pending = handle
                pending.result()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / (a.batches * B) * 1e3

        med, samples = alternate(setups, min(a.rounds, 5), loop)
        base = med[f"plain {W}x{H}"]
        result["step"][precision] = {name: {"wall_ms_per_image": round(ms, 4), "min": round(min(samples[name]), 4), "max": round(max(samples[name]), 4),
                                            "x_plain": round(ms / base, 3)} for name, ms in med.items()}
        print(json.dumps({precision: result["step"][precision]}, indent=1), flush=True)
        del net, setups
    result["note"] = "random-init weights: times only, no accuracy claim"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
