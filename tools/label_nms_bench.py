#!/usr/bin/env python3
"""Cross-label anchor suppression (`--label_nms`), measured in one process on 128 x 128 maps (512 x 512 network input):

  * the plain path of the flag, `sd_nms5` with the sigmoid fused + `sd_label_nms` on the label channels of its output, on the heatmap planes
    of a (B, C + 4, 128, 128) head tensor (channel-slice views, as `LabelNms` passes them), R = 2 and 8: the default label set at B = 64
    and B = 1, and 252 labels + 4 parts at B = 16 and B = 1 (one block per tile and image walks all the labels: few tiles at B = 1 leave
    most CUs idle);
  * beside each: `sd_nms5` alone over the same channels (the pass the flag adds to) and the HBM floor of the task -- input planes read
    once, output planes written once -- at the COPY RATE measured in this process.  (A one-launch form from the logits, `sd_nms5_labels`,
    was timed by an earlier version of this tool against the two launches and not kept: profiles/label_nms_one_launch_ab.json);
  * `sd_label_nms` on the anchor maps of a 3 x 3 tile canvas (352 x 352 cells, B = 16), the path behind the wrappers;
  * `evaluate`-style wall time per image from 2448 x 2048 uint8 sources (preprocess + forward + decode submitted one batch ahead of the
    host assembly, as model/predictor.py does) without and with the flag, in fp32 and `--bf16_inference`.

Kernel times: device events around `--launches` back-to-back launches, the candidates alternated round by round, median over `--rounds`
after a warm-up round.  Wall times: host clock around `--batches` batches ending in a device synchronise, candidates alternated, median.
Random-init weights and random logits: this measures time only and says nothing about accuracy.
usage: label_nms_bench.py [--out profiles/label_nms_bench.json] [--rounds 7] [--launches 50] [--batches 4]"""
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "label_nms_bench.json"))
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--launches", type=int, default=50); ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--skip_steps", action="store_true", help="kernels only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_nms_bench.py measures on the GPU: no device visible")
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import Decoder, preprocess_images
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.tta import with_tta
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = L.lib()
    names = json.loads((ROOT / "labels.json").read_text())
    labels, parts = {n: i for i, n in enumerate(names["labels"])}, {n: i for i, n in enumerate(names["parts"])}
    h = w = 128
    result = {"device": torch.cuda.get_device_name(dev), "map": [h, w], "rounds": a.rounds, "launches_per_sample": a.launches}

    # ---- the copy rate of this device, in this process: what "read once + write once" costs
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    med, _ = alternate({"copy": lambda: dst.copy_(src)}, a.rounds, lambda fn: event_ms(fn, 10))
    copy_gbs = 2 * src.numel() / med["copy"] / 1e6
    result["copy_rate_gbs_measured"] = round(copy_gbs, 1)
    del src, dst

    def report(med, samples, moved):
        return {name: {"us": round(ms * 1e3, 2), "min_us": round(min(samples[name]) * 1e3, 2), "max_us": round(max(samples[name]) * 1e3, 2),
                       "bytes": moved[name], "floor_us_at_copy_rate": round(moved[name] / copy_gbs / 1e3, 2),
                       "x_floor": round(ms * 1e3 / (moved[name] / copy_gbs / 1e3), 2), "achieved_gbs": round(moved[name] / ms / 1e6, 1)}
                for name, ms in med.items()}

    gen = torch.Generator(dev).manual_seed(0)
    result["kernels"] = {}
    for tag, M, N, batches in (("default label set", len(labels), len(parts), (64, 1)), ("252 labels + 4 parts", 252, 4, (16, 1))):
        C = M + N
        for B in batches:
            head = torch.randn(B, C + 4, h, w, device=dev, generator=gen) * 4
            _, p, sb, sc = L.map_view(head[:, :C])
            assert p == head.data_ptr()
            maps = torch.empty(B, C, h, w, device=dev)
            anchors = torch.empty(B, M, h, w, device=dev)
            plane = 4 * B * C * h * w

            def nms5():
                L.check(lib.sd_nms5(p, sb, sc, maps.data_ptr(), B, C, h, w, 1, L.stream()), "sd_nms5")

            def two(R):
                nms5()
                L.check(lib.sd_label_nms(maps.data_ptr(), C * h * w, h * w, anchors.data_ptr(), B, M, h, w, R, L.stream()), "sd_label_nms")
            kernels = {"sd_nms5 sigmoid fused (the pass the flag adds to)": nms5}
            moved = {"sd_nms5 sigmoid fused (the pass the flag adds to)": 2 * plane}
            for R in (2, 8):
                kernels[f"sd_nms5 + sd_label_nms R={R} (two launches)"] = lambda R=R: two(R)
                moved[f"sd_nms5 + sd_label_nms R={R} (two launches)"] = 2 * plane          # the floor of the TASK: logits in, maps out
            med, samples = alternate(kernels, a.rounds, lambda fn: event_ms(fn, a.launches))
            entry = report(med, samples, moved)
            result["kernels"][f"{tag} B={B}"] = entry
            del head, maps, anchors
    # ---- the wrappers' path: sd_label_nms on the anchor maps of a 3 x 3 tile canvas
    B, M = 16, len(labels)
    hc = wc = 3 * 128 - 2 * 16
    merged = torch.rand(B, M + len(parts), hc, wc, device=dev, generator=gen)
    merged = torch.where(merged > 0.96, merged, torch.zeros_like(merged))     # as sparse as a suppressed map (1 cell in 25)
    _, p, sb, sc = L.map_view(merged[:, :M])
    out = torch.empty(B, M, hc, wc, device=dev)
    kernels = {f"sd_label_nms R={R}": (lambda R=R: L.check(lib.sd_label_nms(p, sb, sc, out.data_ptr(), B, M, hc, wc, R, L.stream()), "sd_label_nms"))
               for R in (2, 8)}
    med, samples = alternate(kernels, a.rounds, lambda fn: event_ms(fn, a.launches))
    result["kernels"][f"3x3 tile canvas {hc}x{wc} B={B}"] = report(med, samples, {k: 2 * 4 * B * M * hc * wc for k in kernels})
    del merged, out
    print(json.dumps({"copy_rate_gbs_measured": result["copy_rate_gbs_measured"], "kernels": result["kernels"]}, indent=1), flush=True)

    # ---- the whole step, per image, from camera-sized sources
    result["step"] = {}
    B, W, H = 16, 4 * w, 4 * h
    sources = torch.randint(0, 256, (B, 2048, 2448, 3), dtype=torch.uint8, device=dev, generator=gen)
    for precision, bf16 in (() if a.skip_steps else (("fp32", False), ("bf16_inference", True))):
        def make_args(**kw):
            return Namespace(labels=labels, parts=parts, _r_labels={v: k for k, v in labels.items()}, _r_parts={v: k for k, v in parts.items()},
                             anchor_name="stem", down_ratio=4.0, max_objects=20, max_parts=40, conf_threshold=0.5, decoder_dist_thresh=0.1,
                             fpn_depth=128, bf16_inference=bf16, device=dev, width=W, height=H, **kw)
        torch.manual_seed(0)
        net = Network(make_args(), pretrained=False).to(dev).eval()

        def step(**kw):
            args = make_args(**kw)
            model, decoder = with_tta(net, Decoder(args), args)
            return lambda: decoder.submit(model(preprocess_images(sources, (W, H))), with_raw_parts=True)
        setups = {"plain": step(), "--label_nms 2": step(label_nms=2), "--label_nms 8": step(label_nms=8)}

        def loop(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pending = None
            with torch.no_grad():
                for _ in range(a.batches):
                    handle = fn()
                    if pending is not None:
                        pending.result()
                    pending = handle
                pending.result()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / (a.batches * B) * 1e3

        med, samples = alternate(setups, min(a.rounds, 5), loop)
        result["step"][precision] = {name: {"wall_ms_per_image": round(ms, 4), "min": round(min(samples[name]), 4), "max": round(max(samples[name]), 4),
                                            "x_plain": round(ms / med["plain"], 3)} for name, ms in med.items()}
        print(json.dumps({precision: result["step"][precision]}, indent=1), flush=True)
        del net, setups
    result["note"] = "random-init weights and random logits: times only, no accuracy claim"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
