#!/usr/bin/env python3
"""Flip test-time augmentation, measured in one process at bs = 64 with 128 x 128 maps (512 x 512 input) and the default label set:

  * `sd_tta_merge_nms` for V = 2 and V = 4 on the heatmap planes of a (V*64, 7, 128, 128) head tensor (channel-slice views, as
    `FlipTta` passes them) against its HBM floor of (V + 1) * B * C * h * w * 4 bytes;
  * `RawDecoder`'s `sd_nms5` pass (sigmoid fused) on the planes of view 0: the yardstick that moves 2 * B * C * h * w * 4 bytes;
  * `sd_tta_views` at 64 x 3 x 512 x 512 ((V + 1) * B * 3 * H * W * 4 bytes);
  * `evaluate`-style wall time per image (forward + decode submitted one batch ahead of the host assembly, as model/predictor.py
    does), plain against each `--tta` mode on the same images, fp32 and `--bf16_inference`.

Kernel times: device events around `--launches` back-to-back launches, the candidates alternated round by round, median over `--rounds`
after a warm-up round.  Wall times: host clock around `--batches` batches ending in a device synchronise, modes alternated, median.
Random-init weights: this measures time only and says nothing about accuracy.
usage: tta_bench.py [--out profiles/tta_bench.json] [--rounds 7] [--launches 50] [--batches 6]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from argparse import Namespace
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0            # MI355X nominal HBM3E bandwidth


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tta_bench.json"))
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--launches", type=int, default=50); ap.add_argument("--batches", type=int, default=6)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_bench.py measures on the GPU: no device visible")
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import Decoder
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.tta import VIEW_FLIPS, FlipTta, tta_decoder, tta_views
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = L.lib()
    names = json.loads((ROOT / "labels.json").read_text())
    labels, parts = {n: i for i, n in enumerate(names["labels"])}, {n: i for i, n in enumerate(names["parts"])}
    M, N = len(labels), len(parts)
    B, h, w, nb = 64, 128, 128, M + N
    plane_bytes = B * nb * h * w * 4
    result = {"device": torch.cuda.get_device_name(dev), "batch": B, "map": [h, w], "heatmap_channels": nb, "rounds": a.rounds,
              "launches_per_sample": a.launches, "hbm_peak_gbs_nominal": HBM_PEAK_GBS}

    # ---- the merge against its floor, and the sd_nms5 yardstick, on the same planes
    gen = torch.Generator(dev).manual_seed(0)
    head = torch.randn(4 * B, nb + 4, h, w, device=dev, generator=gen) * 4
    hm, p, sb, sc = L.map_view(head[:, :nb])
    assert p == head.data_ptr()
    out = torch.empty(B, nb, h, w, device=dev)

    def merge(flips):
        fl = (C.c_ubyte * len(flips))(*flips)
        return lambda: L.check(lib.sd_tta_merge_nms(p, sb, sc, out.data_ptr(), B, nb, h, w, len(flips), fl, L.stream()), "sd_tta_merge_nms")

    kernels = {"sd_nms5 (sigmoid fused, RawDecoder's pass)": lambda: L.check(lib.sd_nms5(p, sb, sc, out.data_ptr(), B, nb, h, w, 1, L.stream()), "sd_nms5"),
               "sd_tta_merge_nms V=2": merge(VIEW_FLIPS["hflip"]), "sd_tta_merge_nms V=4": merge(VIEW_FLIPS["hvflip"])}
    moved = {"sd_nms5 (sigmoid fused, RawDecoder's pass)": 2 * plane_bytes, "sd_tta_merge_nms V=2": 3 * plane_bytes, "sd_tta_merge_nms V=4": 5 * plane_bytes}
    med, samples = alternate(kernels, a.rounds, lambda fn: event_ms(fn, a.launches))
    base = med["sd_nms5 (sigmoid fused, RawDecoder's pass)"]
    result["merge"] = {name: {"us": round(ms * 1e3, 2), "min_us": round(min(samples[name]) * 1e3, 2), "max_us": round(max(samples[name]) * 1e3, 2),
                              "bytes": moved[name], "floor_us_at_nominal_hbm": round(moved[name] / HBM_PEAK_GBS / 1e3, 2),
                              "achieved_gbs": round(moved[name] / ms / 1e6, 1), "x_sd_nms5": round(ms / base, 3)} for name, ms in med.items()}
    del head, hm

    # ---- the views
    x = torch.randn(B, 3, 512, 512, device=dev, generator=gen)
    views = {f"sd_tta_views V={len(f)}": (lambda f=f: tta_views(x, f)) for f in (VIEW_FLIPS["hflip"], VIEW_FLIPS["hvflip"])}
    med, samples = alternate(views, a.rounds, lambda fn: event_ms(fn, 10))
    result["views"] = {name: {"us": round(ms * 1e3, 2), "bytes": (int(name[-1]) + 1) * x.numel() * 4,
                              "achieved_gbs": round((int(name[-1]) + 1) * x.numel() * 4 / ms / 1e6, 1)} for name, ms in med.items()}
    print(json.dumps({"merge": result["merge"], "views": result["views"]}, indent=1), flush=True)

    # ---- evaluate-style wall time per image
    result["evaluate"] = {}
    for precision, bf16 in (("fp32", False), ("bf16_inference", True)):
        args = Namespace(labels=labels, parts=parts, _r_labels={v: k for k, v in labels.items()}, _r_parts={v: k for k, v in parts.items()},
                         anchor_name="stem", down_ratio=4.0, max_objects=20, max_parts=40, conf_threshold=0.5, decoder_dist_thresh=0.1,
                         fpn_depth=128, bf16_inference=bf16, device=dev)
        torch.manual_seed(0)
        net = Network(args, pretrained=False).to(dev).eval()
        setups = {"none": (net, Decoder(args))}
        for mode in VIEW_FLIPS:
            setups[mode] = (FlipTta(net, args, mode), tta_decoder(args))

        def loop(setup):
            model, decoder = setup
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pending = None
            with torch.no_grad():
                for _ in range(a.batches):
                    handle = decoder.submit(model(x), with_raw_parts=True)
                    if pending is not None:
                        pending.result()
                    pending = handle
                pending.result()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / (a.batches * B) * 1e3

        def forward_ms(setup):
            with torch.no_grad():
                return event_ms(lambda: setup[0](x), 3) / B

        med, samples = alternate(setups, min(a.rounds, 5), loop)
        fwd, _ = alternate(setups, 3, forward_ms)
        result["evaluate"][precision] = {mode: {"wall_ms_per_image": round(ms, 4), "min": round(min(samples[mode]), 4), "max": round(max(samples[mode]), 4),
                                                "x_plain": round(ms / med["none"], 3), "gpu_forward_and_merge_ms_per_image": round(fwd[mode], 4),
                                                "gpu_x_plain": round(fwd[mode] / fwd["none"], 3)} for mode, ms in med.items()}
        print(json.dumps({precision: result["evaluate"][precision]}, indent=1), flush=True)
        del net, setups
    result["note"] = "random-init weights: times only, no accuracy claim"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
