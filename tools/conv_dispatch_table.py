#!/usr/bin/env python3
"""Table of what the conv host layer decides, for a fixed sweep of descriptors and dispatch options: per case the kernel names
(sd_conv2d_kernel_name passes 0, 1, 2, 16, 17), both sd_conv2d_fwd_bn_stats_rows, every conv workspace size and
sd_conv2d_fwd_bf16_head_supported -- and a sha256 over all lines.  Two builds of the library that print the same sha256 dispatch
alike; a change to the host part of csrc/sd_conv.hip that is meant to be neutral is checked by running this on both.

Needs no GPU: these queries make no HIP call.

    python3 tools/conv_dispatch_table.py [--root CHECKOUT] [--lines]

--root: import structuredetector_amd (and load its built library) from another checkout; --lines: print every line, not only the digest."""
import argparse
import ctypes as C
import hashlib
import sys
from pathlib import Path

# (Cin, Cout, kernel, stride, pad): the conv shapes of the network, its stem, and a 64 -> 64 1x1 that no layer has
CONVS = [(64, 64, 3, 1, 1), (64, 128, 3, 2, 1), (128, 128, 3, 1, 1), (64, 128, 1, 2, 0), (128, 256, 3, 2, 1), (256, 256, 3, 1, 1),
         (128, 256, 1, 2, 0), (256, 512, 3, 2, 1), (512, 512, 3, 1, 1), (256, 512, 1, 2, 0), (512, 128, 1, 1, 0), (256, 128, 1, 1, 0),
         (128, 128, 1, 1, 0), (64, 128, 1, 1, 0), (3, 64, 7, 2, 3), (64, 64, 1, 1, 0)]
BATCHES = (1, 2, 8, 16, 64)
# input maps: square, non-square, not powers of two; the wide ones (few batch sizes) reach the column strips of k_conv3x3_bf16_pp
MAPS = ((8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (256, 256), (24, 32), (96, 128), (128, 80), (40, 40))
WIDE_MAPS = ((64, 512), (16, 1024), (8, 4096), (4, 8192))
DEFAULTS = {"conv_patch_min_tiles": 512, "conv_pp_min_tiles": 200, "conv_rows64_min_units": 192, "conv_rows_f32_min_units": 192,
            "conv_fwd_split_k": 1, "conv_patch_narrow": 2, "conv_pp_strips": 1, "conv_rows16": 1, "igemm_big_bf16": 0,
            "conv1x1_stream_min_pixels": 32 * 2048, "conv_patch_bn64": 0, "wgrad_f32_ring": 2, "wgrad_bf16_ring": 5}
# one option away from the defaults per block of the table
SETTINGS = [None, ("conv_patch_min_tiles", 1), ("conv_pp_min_tiles", 1), ("conv_rows64_min_units", 1), ("conv_rows_f32_min_units", 1),
            ("conv_fwd_split_k", 0), ("conv_patch_narrow", 0), ("conv_patch_narrow", 1), ("conv_pp_strips", 0), ("conv_rows16", 0),
            ("igemm_big_bf16", 1), ("conv1x1_stream_min_pixels", 32), ("conv_patch_bn64", 1), ("wgrad_f32_ring", 0), ("wgrad_f32_ring", 1),
            ("wgrad_bf16_ring", 0), ("wgrad_bf16_ring", 3)]
SIZE_QUERIES = ("sd_conv2d_fwd_workspace_bytes", "sd_conv2d_fwd_bf16_workspace_bytes", "sd_conv2d_fwd_bn_stats_workspace_bytes",
                "sd_conv2d_fwd_bf16_bn_stats_workspace_bytes", "sd_conv2d_dgrad_bn_reduce_workspace_bytes", "sd_conv2d_wgrad_workspace_bytes",
                "sd_conv2d_wgrad_bf16_workspace_bytes")


def table(L):
    lib = L.lib()
    lines = []
    for setting in SETTINGS:
        if setting:
            assert lib.sd_set_option(setting[0].encode(), setting[1]) == 0
        shapes = [(B, H, W) for B in BATCHES for (H, W) in MAPS] + [(B, H, W) for B in (1, 16) for (H, W) in WIDE_MAPS]
        for B, H, W in shapes:
            for cin, cout, k, s, p in CONVS:
                d = L.ConvDesc()
                d.B, d.Hi, d.Wi, d.Cin, d.Cout, d.R, d.S, d.stride, d.pad = B, H, W, cin, cout, k, k, s, p
                d.Ho, d.Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
                if d.Ho < 1 or d.Wo < 1:
                    continue
                r = [setting, B, H, W, cin, cout, k, s]
                r += [lib.sd_conv2d_kernel_name(C.byref(d), w).decode() for w in (0, 1, 2, 16, 17)]
                if cin % 64 == 0:       # the sizes of the entry points that take this conv (the stem has its own)
                    r += [lib.sd_conv2d_fwd_bn_stats_rows(C.byref(d), b) for b in (0, 1)]
                    r += [getattr(lib, q)(C.byref(d)) for q in SIZE_QUERIES]
                    r += [lib.sd_conv2d_fwd_bf16_head_supported(C.byref(d), 7)]
                lines.append(repr(r))
        if setting:
            assert lib.sd_set_option(setting[0].encode(), DEFAULTS[setting[0]]) == 0
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--lines", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    from structuredetector_amd import _lib as L
    lines = table(L)
    if args.lines:
        print("\n".join(lines))
    names = sorted({n for ln in lines for n in eval(ln)[8:13]})
    print(f"{len(lines)} lines, {len(names)} kernels, sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")
    print("kernels:", ", ".join(names))


if __name__ == "__main__":
    main()
