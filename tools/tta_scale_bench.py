#!/usr/bin/env python3
"""Multi-scale test-time augmentation, measured in one process at bs = 64 with a 128 x 128 base map (512 x 512 input) and the default
label set:

  * `sd_tta_scale_merge_nms` for the scale sets {1}, {0.75, 1, 1.25} and {0.5, 0.75, 1, 1.25, 1.5}, each with V = 1, 2 and 4 views, on
    the heatmap planes of (V*64, 7, hs, ws) head tensors (channel-slice views, as `ScaleTta` passes them), against its HBM floor of
    sum_s V*B*C*hs*ws*4 bytes read + B*C*h*w*4 bytes written at the copy rate this process measures on 1 GiB buffers
    (tools/hbm_rw_micro.py's copy);
  * `sd_nms5` (sigmoid fused) and `sd_tta_merge_nms` V = 2, 4 on the same base batch beside it, and every S = 1 candidate TWICE in the
    alternation: the difference between the two copies of one candidate is the run-to-run spread the S = 1 rows are judged against;
  * the whole `ScaleTta` step (resize + normalise of the sources at every size, views, S forwards, merge) as a multiple of the plain
    step (resize + normalise, one forward) in GPU time, fp32 and `--bf16_inference`.

Kernel times: device events around `--launches` back-to-back launches, the candidates alternated round by round, median over `--rounds`
after a warm-up round.  Random-init weights: this measures time only and says nothing about accuracy.
usage: tta_scale_bench.py [--out profiles/tta_scale_bench.json] [--rounds 7] [--launches 50]"""
import argparse
import ctypes as C
import json
import statistics
import sys
from argparse import Namespace
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SCALE_SETS = {"{1}": (), "{0.75,1,1.25}": (0.75, 1.25), "{0.5,0.75,1,1.25,1.5}": (0.5, 0.75, 1.25, 1.5)}
FLIPS = {1: (0,), 2: (0, 1), 4: (0, 1, 2, 3)}


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


def copy_rate_gbs(dev):
    """Read + write rate of a plain copy between two 1 GiB buffers (best of 5 x 5), in GB/s."""
    n = 1 << 28
    a, b = torch.empty(n, device=dev), torch.empty(n, device=dev)
    for _ in range(2):
        b.copy_(a)
    best = min(event_ms(lambda: b.copy_(a), 5) for _ in range(5))
    return 2 * n * 4 / best / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tta_scale_bench.json"))
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_scale_bench.py measures on the GPU: no device visible")
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import preprocess_images
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.tta import ScaleTta, scale_sizes
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = L.lib()
    names = json.loads((ROOT / "labels.json").read_text())
    labels, parts = {n: i for i, n in enumerate(names["labels"])}, {n: i for i, n in enumerate(names["parts"])}
    nb = len(labels) + len(parts)
    B, W, H = 64, 512, 512
    h, w = H // 4, W // 4
    size_args = Namespace(width=W, height=H)
    rate = copy_rate_gbs(dev)
    result = {"device": torch.cuda.get_device_name(dev), "batch": B, "base_map": [h, w], "heatmap_channels": nb, "rounds": a.rounds,
              "launches_per_sample": a.launches, "measured_copy_rate_gbs": round(rate, 1)}

    # ---- the merge against its floor, beside sd_nms5 and sd_tta_merge_nms on the same base batch
    gen = torch.Generator(dev).manual_seed(0)
    all_sizes = scale_sizes(size_args, SCALE_SETS["{0.5,0.75,1,1.25,1.5}"])
    heads = {size: torch.randn(4 * B, nb + 4, size[1] // 4, size[0] // 4, device=dev, generator=gen) * 4 for size in all_sizes}
    out = torch.empty(B, nb, h, w, device=dev)
    base = heads[(W, H)]
    _, p0, sb0, sc0 = L.map_view(base[:, :nb])
    assert p0 == base.data_ptr()
    kernels, moved = {}, {}

    def scale_merge(sizes, V):
        views = [L.map_view(heads[s][:V * B, :nb]) for s in sizes]
        S = len(views)
        assert all(v[1] == heads[s].data_ptr() for v, s in zip(views, sizes))
        arrs = ((C.c_void_p * S)(*[v[1] for v in views]), (C.c_int64 * S)(*[v[2] for v in views]), (C.c_int64 * S)(*[v[3] for v in views]),
                (C.c_int * S)(*[s[1] // 4 for s in sizes]), (C.c_int * S)(*[s[0] // 4 for s in sizes]))
        fl = (C.c_ubyte * V)(*FLIPS[V])
        return lambda: L.check(lib.sd_tta_scale_merge_nms(*arrs, out.data_ptr(), B, nb, h, w, S, V, fl, L.stream()), "sd_tta_scale_merge_nms")

    def flip_merge(V):
        fl = (C.c_ubyte * V)(*FLIPS[V])
        return lambda: L.check(lib.sd_tta_merge_nms(p0, sb0, sc0, out.data_ptr(), B, nb, h, w, V, fl, L.stream()), "sd_tta_merge_nms")

    plane = B * nb * 4
    for rep in ("", " (again)"):
        kernels["sd_nms5 sigmoid fused" + rep] = lambda: L.check(lib.sd_nms5(p0, sb0, sc0, out.data_ptr(), B, nb, h, w, 1, L.stream()), "sd_nms5")
        moved["sd_nms5 sigmoid fused" + rep] = 2 * plane * h * w
        for V in (2, 4):
            kernels[f"sd_tta_merge_nms V={V}" + rep] = flip_merge(V)
            moved[f"sd_tta_merge_nms V={V}" + rep] = (V + 1) * plane * h * w
        for V in (1, 2, 4):
            kernels[f"sd_tta_scale_merge_nms {{1}} V={V}" + rep] = scale_merge([(W, H)], V)
            moved[f"sd_tta_scale_merge_nms {{1}} V={V}" + rep] = (V + 1) * plane * h * w
    for name, ratios in list(SCALE_SETS.items())[1:]:
        sizes = scale_sizes(size_args, ratios)
        for V in (1, 2, 4):
            kernels[f"sd_tta_scale_merge_nms {name} V={V}"] = scale_merge(sizes, V)
            moved[f"sd_tta_scale_merge_nms {name} V={V}"] = plane * (V * sum((s[0] // 4) * (s[1] // 4) for s in sizes) + h * w)
    med, samples = alternate(kernels, a.rounds, lambda fn: event_ms(fn, a.launches))
    result["merge"] = {name: {"us": round(ms * 1e3, 2), "min_us": round(min(samples[name]) * 1e3, 2), "max_us": round(max(samples[name]) * 1e3, 2),
                              "bytes": moved[name], "floor_us_at_measured_copy_rate": round(moved[name] / rate / 1e3, 2),
                              "achieved_gbs": round(moved[name] / ms / 1e6, 1)} for name, ms in med.items()}
    pairs = [n for n in med if n + " (again)" in med]
    result["run_to_run_spread"] = {"between_the_two_copies_of_a_candidate_pct": {n: round(abs(med[n] / med[n + " (again)"] - 1) * 100, 2) for n in pairs},
                                   "max_pct": round(max(abs(med[n] / med[n + " (again)"] - 1) for n in pairs) * 100, 2)}
    both = lambda n: (med[n] + med[n + " (again)"]) / 2
    result["s1_vs_flip_merge_pct"] = {f"V={V}": round((both(f"sd_tta_scale_merge_nms {{1}} V={V}") / both(f"sd_tta_merge_nms V={V}") - 1) * 100, 2) for V in (2, 4)}
    result["s1_v1_vs_nms5_pct"] = round((both("sd_tta_scale_merge_nms {1} V=1") / both("sd_nms5 sigmoid fused") - 1) * 100, 2)
    print(json.dumps({k: result[k] for k in ("measured_copy_rate_gbs", "merge", "run_to_run_spread", "s1_vs_flip_merge_pct", "s1_v1_vs_nms5_pct")}, indent=1), flush=True)
    del heads, base

    # ---- the whole step against the plain step, GPU time
    src = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    result["step"] = {}
    for precision, bf16 in (("fp32", False), ("bf16_inference", True)):
        args = Namespace(labels=labels, parts=parts, fpn_depth=128, bf16_inference=bf16, device=dev, width=W, height=H)
        torch.manual_seed(0)
        net = Network(args, pretrained=False).to(dev).eval()
        steps = {"plain": lambda: net(preprocess_images(src, (W, H)))}
        for name, ratios in list(SCALE_SETS.items())[1:]:
            for mode in ("none", "hvflip"):
                tta = ScaleTta(net, args, scale_sizes(size_args, ratios), mode)
                steps[f"{name} --tta {mode}"] = lambda tta=tta: tta(preprocess_images(src, (W, H)), at_size=lambda size: preprocess_images(src, size))

        def step_ms(fn):
            with torch.no_grad():
                return event_ms(fn, 2)

        med, samples = alternate(steps, 3, step_ms)
        result["step"][precision] = {name: {"gpu_ms_per_batch": round(ms, 3), "min": round(min(samples[name]), 3), "max": round(max(samples[name]), 3),
                                            "x_plain": round(ms / med["plain"], 3)} for name, ms in med.items()}
        print(json.dumps({precision: result["step"][precision]}, indent=1), flush=True)
        del net, steps
        torch.cuda.empty_cache()
    result["note"] = "random-init weights: times only, no accuracy claim"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
