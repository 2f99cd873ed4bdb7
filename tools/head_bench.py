#!/usr/bin/env python3
"""Head (1x1 conv C -> Co, NHWC in, NCHW out) at the bench workload: forward and backward launches, microseconds per call (device events,
warm-up, 20 timed calls) and the share of the binding bound for the algorithmic FLOP and bytes.  Peaks (MI355X_MICROARCH.md): 157.3 TF
fp32 MFMA, 2.5 PF dense bf16 MFMA, 8 TB/s HBM.

  python tools/head_bench.py                                   # bs = 64, 512 x 512 input (128 x 128 head map), C = 128, Co = 7
  python tools/head_bench.py --co 7 --co 64 --co 132 --co 256  # several widths (Co > 32: the GEMM kernels of sd_head_wide.hip)
  python tools/head_bench.py --bf16 --co 64                    # the bf16-activation forward (sd_head_fwd_bf16)"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from structuredetector_amd import _lib as L  # noqa: E402

PEAK_F32, PEAK_BF16, PEAK_HBM = 157.3e12, 2.5e15, 8e12


def timed(fn, name, calls=20, warmup=3):
    for _ in range(warmup):
        L.check(fn(), name)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        L.check(fn(), name)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def report(name, us, flop, nbytes, peak_flop):
    t_flop, t_mem = flop / peak_flop, nbytes / PEAK_HBM
    bound, floor = ("MFMA", t_flop) if t_flop >= t_mem else ("HBM", t_mem)
    print(f"{name:44s} {us:9.1f} us  {flop / 1e9:8.1f} GFLOP {nbytes / 1e6:8.1f} MB  floor {floor * 1e6:7.1f} us ({bound})  "
          f"{floor * 1e6 / us * 100:5.1f} % of the {bound} bound", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--H", type=int, default=128, help="head map height (input / 4)")
    ap.add_argument("--W", type=int, default=128)
    ap.add_argument("--C", type=int, default=128, help="head input depth (fpn_depth)")
    ap.add_argument("--co", type=int, action="append", help="output channels (M + N + 4); repeat for several; default 7")
    ap.add_argument("--bf16", action="store_true", help="time sd_head_fwd_bf16 (bf16 activation) instead of the fp32 passes")
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    lib = L.lib(); dev = "cuda"
    B, H, W, C = a.B, a.H, a.W, a.C
    P = B * H * W
    x = torch.randn(B, H, W, C, device=dev)
    x16 = x.to(torch.bfloat16) if a.bf16 else None
    dx = None if a.bf16 else torch.empty_like(x)
    print(f"head B={B} map {H}x{W} (P = {P} pixels) C={C}" + (" bf16 activation" if a.bf16 else " fp32"), flush=True)
    for Co in a.co or [7]:
        w = torch.randn(Co, C, device=dev) / C ** 0.5; b = torch.randn(Co, device=dev)
        y = torch.empty(B, Co, H, W, device=dev)
        if a.bf16:
            fwd = lambda: lib.sd_head_fwd_bf16(x16.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), B, H * W, C, Co, L.stream())
            us = timed(fwd, "sd_head_fwd_bf16", a.calls)
            report(f"Co={Co:3d} bf16 forward", us, 2 * 2 * P * C * Co, P * (2 * C + 4 * Co), PEAK_BF16)     # (hi + lo: two products)
            continue
        dy = torch.randn(B, Co, H, W, device=dev)
        dw = torch.empty_like(w); db = torch.empty_like(b)
        ws = torch.empty(lib.sd_head_bwd_workspace_bytes(B, H * W, C, Co), dtype=torch.uint8, device=dev)
        fwd = lambda: lib.sd_head_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), B, H * W, C, Co, L.stream())
        bwd = lambda: lib.sd_head_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), B, H * W, C, Co, 0,
                                      ws.data_ptr(), ws.numel(), L.stream())
        us = timed(fwd, "sd_head_fwd", a.calls)
        report(f"Co={Co:3d} fp32 forward", us, 2 * P * C * Co, P * 4 * (C + Co), PEAK_F32)
        us = timed(bwd, "sd_head_bwd", a.calls)
        report(f"Co={Co:3d} fp32 backward (wgrad + dgrad + finalize)", us, 4 * P * C * Co, P * 4 * (2 * C + 2 * Co), PEAK_F32)
        del dy, ws


if __name__ == "__main__":
    main()
