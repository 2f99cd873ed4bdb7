#!/usr/bin/env python3
"""GPU time of the random perspective augmentation (`train --aug_perspective`), bs = 64, network input 512x512.  Device events around
`--reps` calls; every round times every variant once, one after the other, so the variants of a comparison share the round's conditions;
us per call, best round, and the spread (min .. max over the rounds).  Every timed call is the C entry point alone: tables are uploaded once.

1. `sd_perspective_u8` alone on (64, 512, 512, 3) bytes -- with the similarity rows `--aug_rotate 30 --aug_scale 0.2 --aug_translate 0.1` draws,
   padded with a6 = a7 = 0, and with those rows folded into the homographies `--aug_perspective 0.3` draws -- beside its HBM floor, 6 B per
   pixel (3 read, 3 written) at the copy rate `tools/hbm_rw_micro.py` measures (a 1 GiB fp32 `copy_`, read + write), taken in this process.
2. The training chain (ColorJitter + flips, packed) from 512x512 and from 2448x2048 sources: no warp, the affine warp (k_affine_u8), the same
   rows through the perspective form (k_persp_u8: the only difference is the two divisions), and the perspective draw.  warp - off is the
   added launch.
3. With `--parent-root` (a built checkout of the parent commit) the no-warp and the affine chain also run through the PARENT's library,
   loaded beside this one, through the same entry point and inside the same rounds: the flag-off chain and k_affine_u8 against the parent,
   next to the parent's own spread.

Writes one JSON document (default profiles/perspective_bench.json)."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--label", type=str, default="")
ap.add_argument("--parent-root", type=Path, default=None)
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "perspective_bench.json")
opt = ap.parse_args()

sys.path.insert(0, str(ROOT))
from structuredetector_amd import _lib as L  # noqa: E402
from structuredetector_amd.data.augment import (_FILL, _MEAN, _STD, _tables, _upload, affine_inverse_matrix, compose_affine_perspective,  # noqa: E402
                                                jitter_words, perspective_coeffs)

dev = torch.device("cuda", torch.cuda.current_device())
rng = np.random.default_rng(0)
B, size = opt.batch, (512, 512)
Wout, Hout = size
flips = [int(v) for v in rng.integers(0, 4, B)]
words, factors = zip(*(jitter_words(list(rng.permutation(4)), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.85, 1.15),
                                    rng.uniform(-0.05, 0.05)) for _ in range(B)))
jitter = (list(words), list(factors))
affine = [affine_inverse_matrix(size, rng.uniform(-30, 30), rng.uniform(0.8, 1.2), (rng.uniform(-51.2, 51.2), rng.uniform(-51.2, 51.2)))
          for _ in range(B)]
similarity8 = [list(m) + [0.0, 0.0] for m in affine]                            # the same rows for k_persp_u8
frame = [(0.0, 0.0), (float(Wout), 0.0), (float(Wout), float(Hout)), (0.0, float(Hout))]
D = 0.3
policy8 = []
for m in affine:                                                                # TrainAugmentation's policy with numpy's uniforms
    u = rng.uniform(0, 1, 9)
    hw, hh = D * Wout / 2, D * Hout / 2
    quad = [(u[1] * hw, u[2] * hh), (Wout - u[3] * hw, u[4] * hh), (Wout - u[5] * hw, Hout - u[6] * hh), (u[7] * hw, Hout - u[8] * hh)]
    policy8.append(compose_affine_perspective(m, perspective_coeffs(frame, quad) if u[0] < 0.5 else [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]))


def load_parent(root):
    """The parent commit's library beside this one (its symbols stay local to the handle), with this package's signatures."""
    handle = C.CDLL(str(root / "structuredetector_amd" / "csrc" / "libsdnet_hip.so"))
    for name in ("sd_preprocess_images_blur",):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = L._SIGNATURES[name]
    return handle


def run_rounds(variants, reps):
    """{name: (best, worst) us per call}: a warm-up of every variant, then `--rounds` rounds of every variant in turn, the order reversed
    in every other round so that no variant always runs behind the same neighbour."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    seen = {name: [] for name in variants}
    for k in range(opt.rounds):
        for name, fn in (list(variants.items())[::-1] if k & 1 else variants.items()):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            seen[name].append(e0.elapsed_time(e1) / reps * 1e3)
    return {name: (min(v), max(v)) for name, v in seen.items()}


lib = L.lib()
parent = load_parent(opt.parent_root.resolve()) if opt.parent_root is not None else None
doc = {"tool": "tools/perspective_bench.py", "label": opt.label, "device": torch.cuda.get_device_name(0), "reps": opt.reps, "rounds": opt.rounds,
       "batch": B, "out": "512x512", "aug_perspective": D, "parent": None if parent is None else "the parent commit's library, same process and rounds"}

a = torch.empty(1 << 28, device=dev)
b = torch.empty(1 << 28, device=dev)
best, worst = run_rounds({"copy": lambda: b.copy_(a)}, 5)["copy"]
copy_tbs = 2 * (1 << 30) / 1e12 / (best * 1e-6)
doc["hbm_copy"] = {"what": "1 GiB fp32 copy_ (read + write), the measurement of tools/hbm_rw_micro.py", "us": round(best, 1),
                   "tb_per_s": round(copy_tbs, 3)}
print(json.dumps(doc["hbm_copy"]), flush=True)
del a, b

# 1. the stand-alone stage
img = torch.from_numpy(rng.integers(0, 256, (B, Hout, Wout, 3), dtype=np.uint8)).to(dev)
dst = torch.empty_like(img)
fill = (C.c_ubyte * 3)(*_FILL)
floor_bytes = 2 * img.numel()
floor_us = floor_bytes / (copy_tbs * 1e12) * 1e6
tables = {"similarity": torch.tensor(np.asarray(similarity8), device=dev), "policy": torch.tensor(np.asarray(policy8), device=dev)}
stage = run_rounds({name: (lambda t=t: L.check(lib.sd_perspective_u8(img.data_ptr(), dst.data_ptr(), B, Hout, Wout, t.data_ptr(), fill, L.stream()),
                                               "sd_perspective_u8")) for name, t in tables.items()}, 50)
doc["stage"] = []
for name, (best, worst) in stage.items():
    row = {"entry": "sd_perspective_u8", "kernel": "k_persp_u8", "rows": name, "us_per_call": round(best, 1), "spread_us": [round(best, 1), round(worst, 1)],
           "hbm_floor_bytes": floor_bytes, "hbm_floor_us_at_copy_rate": round(floor_us, 1), "reached_fraction_of_floor": round(floor_us / best, 3),
           "tb_per_s": round(floor_bytes / 1e12 / (best * 1e-6), 3)}
    doc["stage"].append(row)
    print(json.dumps(row), flush=True)
del img, dst


# 2. and 3. the chain
def chain_call(handle, name, x, rows6=None, rows8=None):
    """One closure per variant: every table on the device already, the call is the entry point alone (packed form, plain resize)."""
    Bn, Hin, Win, _ = x.shape
    hb, hk, hks = _tables.get(Win, Wout, dev)
    vb, vk, vks = _tables.get(Hin, Hout, dev)
    fl, order, fac = _upload("flips", flips, Bn, dev), _upload("jitter_order", jitter[0], Bn, dev), _upload("jitter_factors", jitter[1], Bn, dev)
    rows = None if rows6 is None else _upload("affine", rows6, Bn, dev)
    homography = None if rows8 is None else torch.tensor(np.asarray(rows8), device=dev)
    out = torch.empty((Bn, 3, Hout, Wout), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.sd_preprocess_blur_workspace_bytes(0, Bn, Hin, Win, 0, Hout, Wout, 0), dtype=torch.uint8, device=dev)
    mean, std = (C.c_float * 3)(*_MEAN), (C.c_float * 3)(*_STD)
    ptr = lambda t: t.data_ptr() if t is not None else None
    warp = [ptr(rows), ptr(homography)] if name.endswith("_persp") else [ptr(rows)]
    keep = (hb, hk, vb, vk, fl, order, fac, rows, homography, out, ws, mean, std)
    fn = getattr(handle, name)

    def call(_keep=keep):
        rc = fn(x.data_ptr(), 0, Bn, Hin, Win, 0, 0, Hout, Wout, 0, 0, hb.data_ptr(), hk.data_ptr(), hks, vb.data_ptr(), vk.data_ptr(), vks, None,
                fl.data_ptr(), order.data_ptr(), fac.data_ptr(), *warp, None, None, None, fill, mean, std, out.data_ptr(), ws.data_ptr(), ws.numel(),
                L.stream())
        assert rc == 0, (name, rc)
    return call, out


doc["chain"] = []
for (H, W) in ((512, 512), (2048, 2448)):
    x = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    made = {"off": chain_call(lib, "sd_preprocess_images_blur", x), "affine": chain_call(lib, "sd_preprocess_images_blur", x, rows6=affine),
            "persp_similarity": chain_call(lib, "sd_preprocess_images_persp", x, rows8=similarity8),
            "persp_policy": chain_call(lib, "sd_preprocess_images_persp", x, rows8=policy8)}
    if parent is not None:
        made["parent_off"] = chain_call(parent, "sd_preprocess_images_blur", x)
        made["parent_affine"] = chain_call(parent, "sd_preprocess_images_blur", x, rows6=affine)
    for fn, _ in made.values():
        fn()
    torch.cuda.synchronize()
    same = {"persp_similarity == affine": torch.equal(made["persp_similarity"][1], made["affine"][1])}
    if parent is not None:
        same["off == parent_off"] = torch.equal(made["off"][1], made["parent_off"][1])
        same["affine == parent_affine"] = torch.equal(made["affine"][1], made["parent_affine"][1])
    assert all(same.values()), same
    times = run_rounds({name: fn for name, (fn, _) in made.items()}, opt.reps)
    row = {"source": f"{W}x{H}", "form": "packed", "chain": "jitter_flips", "outputs_equal": same,
           "us_per_call": {name: round(best, 1) for name, (best, _) in times.items()},
           "spread_us": {name: [round(best, 1), round(worst, 1)] for name, (best, worst) in times.items()},
           "k_affine_u8_added_us": round(times["affine"][0] - times["off"][0], 1),
           "k_persp_u8_same_rows_added_us": round(times["persp_similarity"][0] - times["off"][0], 1),
           "aug_perspective_minus_affine_flags_us": round(times["persp_policy"][0] - times["affine"][0], 1),
           "warp_hbm_floor_us_at_copy_rate": round(floor_us, 1)}
    if parent is not None:
        row["off_minus_parent_off_us"] = round(times["off"][0] - times["parent_off"][0], 1)
        row["affine_minus_parent_affine_us"] = round(times["affine"][0] - times["parent_affine"][0], 1)
        row["parent_spread_us"] = {"off": round(times["parent_off"][1] - times["parent_off"][0], 1),
                                   "affine": round(times["parent_affine"][1] - times["parent_affine"][0], 1)}
    doc["chain"].append(row)
    print(json.dumps(row), flush=True)
    del made, x
opt.out.parent.mkdir(parents=True, exist_ok=True)
opt.out.write_text(json.dumps(doc, indent=1) + "\n")
