#!/usr/bin/env python3
"""Transposed views, measured in one process at bs = 64 with 128 x 128 maps (512 x 512 input) and the default label set:

  * `sd_d4_views` for Vf = 1, 2, 4 at 64 x 3 x 512 x 512 ((2 Vf + 1) * B * 3 * H * W * 4 bytes), each beside `sd_tta_views` at the same Vf
    ((Vf + 1) planes; it has no Vf = 1 form: a plain copy stands in);
  * `sd_d4_merge_nms` for Vf = 1, 2, 4 on the heatmap planes of two (Vf*64, 7, 128, 128) head tensors (channel-slice views, as
    `TransposeTta` passes them), each beside `sd_tta_merge_nms` over the SAME number of views (2 Vf = 2, 4; there is no 8-view flip merge):
    the two move the same bytes, the ratio is what the detour of the transposed planes through LDS costs;
  * `sd_transpose_select` on the 64 x 3 x 512 x 512 batch (all copied, all transposed, every other image) in GB/s, beside the
    read-and-write rate of a plain device copy of the same buffer and of 1 GiB (the `copy` line of tools/hbm_rw_micro.py);
  * the whole test step (views + forward(s) + merge, GPU time per image) for plain, `--tta hvflip`, `--tta_transpose` and
    `--tta_transpose --tta hvflip` (8 views) on the same images, fp32.

Kernel times: device events around `--launches` back-to-back launches, the candidates alternated round by round, median over `--rounds`
after a warm-up round.  Random-init weights: this measures time only and says nothing about accuracy.
usage: d4_bench.py [--out profiles/d4_bench.json] [--rounds 7] [--launches 50] [--skip_step]"""
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


def rows(med, samples, moved):
    return {name: {"us": round(ms * 1e3, 2), "min_us": round(min(samples[name]) * 1e3, 2), "max_us": round(max(samples[name]) * 1e3, 2),
                   "bytes": moved[name], "achieved_gbs": round(moved[name] / ms / 1e6, 1)} for name, ms in med.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "d4_bench.json"))
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip_step", action="store_true", help="kernels only: leave out the whole-step comparison")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("d4_bench.py measures on the GPU: no device visible")
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data.augment import transpose_select
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.tta import VIEW_FLIPS, FlipTta, TransposeTta
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = L.lib()
    names = json.loads((ROOT / "labels.json").read_text())
    labels, parts = {n: i for i, n in enumerate(names["labels"])}, {n: i for i, n in enumerate(names["parts"])}
    nb = len(labels) + len(parts)
    B, H, W, h, w = 64, 512, 512, 128, 128
    flips_of = {1: (0,), 2: VIEW_FLIPS["hflip"], 4: VIEW_FLIPS["hvflip"]}
    ub = lambda f: (C.c_ubyte * len(f))(*f)
    result = {"device": torch.cuda.get_device_name(dev), "batch": B, "input": [H, W], "map": [h, w], "heatmap_channels": nb, "rounds": a.rounds,
              "launches_per_sample": a.launches}
    gen = torch.Generator(dev).manual_seed(0)

    # ---- views
    x = torch.randn(B, 3, H, W, device=dev, generator=gen)
    image_bytes = x.numel() * 4
    buf = torch.empty(8 * B, 3, H, W, device=dev)
    cands, moved = {}, {}
    for Vf, f in flips_of.items():
        n = Vf * x.numel()
        cands[f"sd_d4_views Vf={Vf}"] = lambda Vf=Vf, f=f, n=n: L.check(lib.sd_d4_views(x.data_ptr(), buf.data_ptr(), buf.data_ptr() + 4 * n, B, H, W, Vf,
                                                                                       ub(f), L.stream()), "sd_d4_views")
        moved[f"sd_d4_views Vf={Vf}"] = (2 * Vf + 1) * image_bytes
        if Vf > 1:
            cands[f"sd_tta_views V={Vf}"] = lambda Vf=Vf, f=f: L.check(lib.sd_tta_views(x.data_ptr(), buf.data_ptr(), B, H, W, Vf, ub(f), L.stream()),
                                                                      "sd_tta_views")
        else:
            cands["copy (stands in for sd_tta_views V=1)"] = lambda: buf[:B].copy_(x)
        moved[f"sd_tta_views V={Vf}" if Vf > 1 else "copy (stands in for sd_tta_views V=1)"] = (Vf + 1) * image_bytes
    med, samples = alternate(cands, a.rounds, lambda fn: event_ms(fn, 10))
    result["views"] = rows(med, samples, moved)
    print(json.dumps({"views": result["views"]}, indent=1), flush=True)

    # ---- transpose_select against the copy rate
    out = buf[:B]
    sels = {"none selected (copy)": [0] * B, "all selected": [1] * B, "every other image": [i & 1 for i in range(B)]}
    cands = {f"sd_transpose_select, {k}": (lambda s=torch.tensor(v, dtype=torch.uint8, device=dev): L.check(
        lib.sd_transpose_select(x.data_ptr(), out.data_ptr(), B, 3, H, s.data_ptr(), L.stream()), "sd_transpose_select")) for k, v in sels.items()}
    cands["torch copy of the same batch"] = lambda: out.copy_(x)
    moved = {k: 2 * image_bytes for k in cands}
    big_a, big_b = torch.empty(1 << 28, device=dev), torch.empty(1 << 28, device=dev)
    cands["torch copy of 1 GiB (hbm_rw_micro.py's copy)"] = lambda: big_b.copy_(big_a)
    moved["torch copy of 1 GiB (hbm_rw_micro.py's copy)"] = 2 * big_a.numel() * 4
    med, samples = alternate(cands, a.rounds, lambda fn: event_ms(fn, 10))
    result["transpose_select"] = rows(med, samples, moved)
    del big_a, big_b
    assert torch.equal(transpose_select(x, sels["every other image"])[1], x[1].transpose(-1, -2))
    print(json.dumps({"transpose_select": result["transpose_select"]}, indent=1), flush=True)
    del buf, out

    # ---- merges over the same number of views
    head = torch.randn(4 * B, nb + 4, h, w, device=dev, generator=gen) * 4
    head_t = torch.randn(4 * B, nb + 4, w, h, device=dev, generator=gen) * 4
    _, p, sb, sc = L.map_view(head[:, :nb])
    _, pt, sbt, sct = L.map_view(head_t[:, :nb])
    assert p == head.data_ptr() and pt == head_t.data_ptr()
    merged = torch.empty(B, nb, h, w, device=dev)
    plane_bytes = B * nb * h * w * 4
    cands, moved = {}, {}
    for Vf, f in flips_of.items():
        cands[f"sd_d4_merge_nms Vf={Vf}"] = lambda Vf=Vf, f=f: L.check(lib.sd_d4_merge_nms(p, sb, sc, pt, sbt, sct, merged.data_ptr(), B, nb, h, w, Vf, ub(f),
                                                                                          L.stream()), "sd_d4_merge_nms")
        moved[f"sd_d4_merge_nms Vf={Vf}"] = (2 * Vf + 1) * plane_bytes
    for V, f in ((2, VIEW_FLIPS["hflip"]), (4, VIEW_FLIPS["hvflip"])):
        cands[f"sd_tta_merge_nms V={V}"] = lambda V=V, f=f: L.check(lib.sd_tta_merge_nms(p, sb, sc, merged.data_ptr(), B, nb, h, w, V, ub(f), L.stream()),
                                                                   "sd_tta_merge_nms")
        moved[f"sd_tta_merge_nms V={V}"] = (V + 1) * plane_bytes
    med, samples = alternate(cands, a.rounds, lambda fn: event_ms(fn, a.launches))
    result["merge"] = rows(med, samples, moved)
    for Vf, V in ((1, 2), (2, 4)):
        result["merge"][f"sd_d4_merge_nms Vf={Vf}"]["x_sd_tta_merge_nms_same_views"] = round(med[f"sd_d4_merge_nms Vf={Vf}"] / med[f"sd_tta_merge_nms V={V}"], 3)
    print(json.dumps({"merge": result["merge"]}, indent=1), flush=True)
    del head, head_t

    # ---- the whole step
    if not a.skip_step:
        args = Namespace(labels=labels, parts=parts, _r_labels={v: k for k, v in labels.items()}, _r_parts={v: k for k, v in parts.items()},
                         anchor_name="stem", down_ratio=4.0, max_objects=20, max_parts=40, conf_threshold=0.5, decoder_dist_thresh=0.1,
                         fpn_depth=128, bf16_inference=False, device=dev)
        torch.manual_seed(0)
        net = Network(args, pretrained=False).to(dev).eval()
        setups = {"plain forward": net, "--tta hvflip (4 views)": FlipTta(net, args, "hvflip"), "--tta_transpose (2 views)": TransposeTta(net, args, "none"),
                  "--tta_transpose --tta hvflip (8 views)": TransposeTta(net, args, "hvflip")}

        def step_ms(model):
            with torch.no_grad():
                return event_ms(lambda: model(x), 2) / B

        med, samples = alternate(setups, 3, step_ms)
        result["step"] = {k: {"gpu_ms_per_image": round(ms, 4), "min": round(min(samples[k]), 4), "max": round(max(samples[k]), 4),
                              "x_plain": round(ms / med["plain forward"], 3)} for k, ms in med.items()}
        print(json.dumps({"step": result["step"]}, indent=1), flush=True)
    result["note"] = "random-init weights: times only, no accuracy claim"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
