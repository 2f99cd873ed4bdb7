#!/usr/bin/env python3
"""Table of what the decoder host layer decides, for a fixed sweep of geometries and decoder options, and a sha256 over its lines.
Per case the OLD columns -- sd_decode_workspace_bytes, sd_decode_fused_workspace_bytes, sd_decode_state_bytes, sd_decode_packed_words,
sd_decode_fused_supported, sd_decode_fused_recommended without and with the exact top-k -- and the NEW ones: sd_decode_kernel_names for
sd_decode (exact top-k and annotations-only, planes vector-loadable and not) and for sd_decode_fused (both modes, without and with the
override bit).  One digest covers the old columns, one all of them; a library without sd_decode_kernel_names gets the first only.  Two
builds that print the same digests dispatch alike: a change to the host part of csrc/sd_decode.hip that is meant to be neutral is
checked by running this on both.  Needs no GPU: these queries make no HIP call.

    python3 tools/decode_dispatch_table.py [--root CHECKOUT] [--lines]
    python3 tools/decode_dispatch_table.py --run [--root CHECKOUT]        (GPU)

--root: import structuredetector_amd (and load its built library) from another checkout; --lines: print every line, not only the digests.

The `lds=` figure of a kernel-names line is the DYNAMIC LDS the launch asks for (the third launch argument).  The LDS_Block_Size column
of a `rocprofv3 --kernel-trace` is another figure: the kernel's static __shared__ arrays, rounded up to 512 bytes, whatever the launch
adds -- compare it with the kernel's .group_segment_fixed_size; the dynamic part is not in that trace.

--run decodes one seeded noise head per case of a small sweep (every option block; shapes the GPU tests decode) through sd_decode and,
where sd_decode_fused_supported says so, through sd_decode_fused with the override bit, in both modes; it prints the sha256 of each
packed buffer and, where the library has it, the kernel-names line of the call.  Each case runs once, in this process; the first error
stops the run.  Under `rocprofv3 --kernel-trace` the trace of this run is the launch sequence those lines describe."""
import argparse
import hashlib
import sys
from pathlib import Path

BATCHES = (1, 2, 8, 16, 20, 32, 54, 64, 96, 128, 130, 256, 300, 512)
MAPS = ((33, 33), (52, 52), (64, 64), (66, 66), (100, 100), (128, 128), (132, 132), (96, 128), (128, 80), (112, 256), (256, 256), (512, 512))
MNKP = ((2, 1, 20, 40), (1, 1, 3, 2), (3, 2, 12, 24), (2, 2, 64, 200), (1, 2, 900, 1000), (8, 8, 128, 512), (64, 64, 16, 16), (65, 1, 20, 40))
# (B, h, w, (M, N, K, P)) of --run
RUN_CASES = [(b, 128, 128, (2, 1, 20, 40)) for b in (1, 16, 64, 130)] + [(2, 256, 256, (8, 8, 128, 512)), (3, 66, 66, (3, 2, 12, 24)),
                                                                           (2, 112, 256, (2, 2, 64, 96))]
DEFAULTS = {"tall_tiles_from": 2688, "map_parallel_from": -1, "map_rows11": 1, "map_stream": 1, "map_tile_height": 0, "map_scalar_nms": 0,
            "map_split": 0, "map_half": 1, "map_waves3": 1, "map_rank_group": 1}
# every value of every key that the tests or the tools set
VALUES = [("map_parallel_from", 1), ("map_parallel_from", 1 << 30), ("tall_tiles_from", 1), ("tall_tiles_from", 1 << 30),
          ("map_tile_height", 16), ("map_tile_height", 32), ("map_scalar_nms", 1), ("map_stream", 0), ("map_split", 1), ("map_split", 2),
          ("map_split", 3), ("map_split", 4), ("map_rank_group", 0), ("map_rank_group", 2), ("map_half", 0), ("map_waves3", 0),
          ("map_waves3", 2), ("map_rows11", 0), ("map_rows11", 8), ("map_rows11", 11)]
# one option away from the defaults per block; most knobs only act on the map-parallel path, so the map_* blocks come with
# map_parallel_from = 1 as well
SETTINGS = [()] + [(kv,) for kv in VALUES] + [(kv, ("map_parallel_from", 1)) for kv in VALUES[4:]]


def kernel_names(lib):
    try:
        return lib.sd_decode_kernel_names
    except AttributeError:      # a library from before the query
        return None


def blocks(lib):
    """Yields each block's settings with the options set, and restores the defaults after the block."""
    for setting in SETTINGS:
        for k, v in setting:
            assert lib.sd_decode_set_option(k.encode(), v) == 0
        yield setting
        for k, _ in setting:
            assert lib.sd_decode_set_option(k.encode(), DEFAULTS[k]) == 0


def table(lib):
    names = kernel_names(lib)
    old, new = [], []
    for setting in blocks(lib):
        for B in BATCHES:
            for h, w in MAPS:
                for M, N, K, P in MNKP:
                    g = (B, M, N, h, w, K, P)
                    r = [setting, *g, lib.sd_decode_workspace_bytes(*g), lib.sd_decode_fused_workspace_bytes(*g),
                         lib.sd_decode_state_bytes(B, M, N, h, w), lib.sd_decode_packed_words(B, K, P), lib.sd_decode_fused_supported(*g),
                         lib.sd_decode_fused_recommended(*g, 0), lib.sd_decode_fused_recommended(*g, 1)]
                    old.append(repr(r))
                    if names:
                        r += [names(*g, exact, vec).decode() for exact in (1, 0) for vec in (1, 0)]
                        r += [names(*g, exact, 2).decode() for exact in (0, 1, 2, 3)]
                        new.append(repr(r))
    return old, new


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def run(L):
    import torch
    lib = L.lib()
    names = kernel_names(lib)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    heads = {}
    for setting in blocks(lib):
        for B, h, w, (M, N, K, P) in RUN_CASES:
            g = (B, M, N, h, w, K, P)
            if g not in heads:
                heads[g] = torch.randn(B, M + N + 4, h, w, generator=gen).to(dev)
            head = heads[g]
            views = [L.map_view(head[:, a:b]) for a, b in ((0, M), (M, M + N), (M + N, M + N + 2), (M + N + 2, M + N + 4))]
            maps = [x for (_, ptr, sb, sc) in views for x in (ptr, sb, sc)]
            conf, dist = 0.5, float(0.1 * min(h, w))
            calls = [("sd_decode", exact, 0) for exact in (1, 0)]
            if lib.sd_decode_fused_supported(*g):
                calls += [("sd_decode_fused", exact | 2, 2) for exact in (1, 0)]
            for entry, exact, flags in calls:
                packed = torch.zeros(lib.sd_decode_packed_words(B, K, P), dtype=torch.int32, device=dev)
                if entry == "sd_decode":
                    ws = L.workspace(lib.sd_decode_workspace_bytes(*g), dev)
                    rc = lib.sd_decode(*maps, *g, conf, dist, exact, packed.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())
                    flags |= 1 if all(ptr % 16 == 0 and sb % 4 == 0 and sc % 4 == 0 for (_, ptr, sb, sc) in views[:2]) else 0
                else:
                    ws = L.workspace(lib.sd_decode_fused_workspace_bytes(*g), dev)
                    state = L.zero_state(lib.sd_decode_state_bytes(B, M, N, h, w), dev, "decode_dispatch_table")
                    rc = lib.sd_decode_fused(*maps, *g, conf, dist, exact, packed.data_ptr(), state.data_ptr(), state.numel(), ws.data_ptr(),
                                             ws.numel(), L.stream())
                L.check(rc, entry)
                torch.cuda.synchronize()
                line = [setting, entry, *g, exact, hashlib.sha256(packed.cpu().numpy().tobytes()).hexdigest()]
                if names:
                    line.append(names(*g, exact, flags).decode())
                print(repr(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--run", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    from structuredetector_amd import _lib as L
    if args.run:
        return run(L)
    old, new = table(L.lib())
    if args.lines:
        print("\n".join(new or old))
    print(f"{len(old)} lines, old columns sha256 {digest(old)}")
    if new:
        print(f"{len(new)} lines, all columns sha256 {digest(new)}")


if __name__ == "__main__":
    main()
