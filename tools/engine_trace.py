#!/usr/bin/env python3
"""Launch trace and result digest of the network engine (`_Engine` of structuredetector_amd/model/network.py) over a fixed set of
configurations: every eval and training schedule the engine has, at the smallest legal input.

  record [--out tests/golden/engine_launch_trace.json]   write the fixture: per configuration the call count, the per-symbol counts, a
                                                         sha256 of the trace text and 16 bits of every line's own digest.  Run it on a
                                                         checkout of the commit the code under test must equal (--root), never on that code.
  diff [--dump DIR]                                      recompute and list every call that differs from the fixture
  digest [--out FILE]                                    sha256 of the head output and, for the training steps, of the gradients and of the
                                                         BatchNorm running buffers (fixed seeds): equal bits between two checkouts

--root DIR: the checkout whose `structuredetector_amd` is traced (default: this one); the recorder always comes from this tree's
tests/helpers.py."""
import argparse
import hashlib
import importlib.util
import json
import sys
from argparse import Namespace
from collections import Counter
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
FIXTURE = HERE / "tests" / "golden" / "engine_launch_trace.json"

# name: (schedule, (B, H, W), engine attributes, bn_sync).  64x64 is the smallest legal input: layer4 is 2x2 and every block, downsample,
# lateral and half-size-residual branch is taken.
CONFIGS = {
    "eval_f32_b2": ("eval", (2, 64, 96), {}, False),
    "eval_f32_b1_sb": ("eval", (1, 64, 64), {"small_batch_kernel": True}, False),
    "eval_f32_b1_no_sb": ("eval", (1, 64, 64), {"small_batch_kernel": False}, False),
    "eval_bf16_b2_fuse_head": ("eval_bf16", (2, 64, 96), {"fuse_head": True}, False),
    "eval_bf16_b2_no_fuse_head": ("eval_bf16", (2, 64, 96), {"fuse_head": False}, False),
    "eval_bf16_b1": ("eval_bf16", (1, 64, 64), {}, False),
    "train_f32": ("train", (2, 64, 64), {}, False),
    "train_f32_fuse_bn_bwd": ("train", (2, 64, 64), {"fuse_bn_bwd": True}, False),
    "train_amp": ("train_amp", (2, 64, 64), {}, False),
    "train_amp_no_stem_ring": ("train_amp", (2, 64, 64), {"stem_ring": False}, False),
    "train_f32_sync": ("train", (2, 64, 64), {}, True),
    "train_amp_sync": ("train_amp", (2, 64, 64), {}, True),
    "train_f32_fuse_bn_bwd_sync": ("train", (2, 64, 64), {"fuse_bn_bwd": True}, True),
    "train_f32_overlap_wgrad": ("train", (2, 64, 64), {"overlap_wgrad": True}, False),
    "train_f32_prof": ("train", (2, 64, 64), {"prof": [], "prof_shapes": []}, False),
}


def _helpers():
    spec = importlib.util.spec_from_file_location("engine_trace_helpers", HERE / "tests" / "helpers.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_config(name, record=True):
    """One configuration on a fresh Network -> (trace lines or None, {what: sha256 of the result bits})."""
    import torch

    from structuredetector_amd import _lib as L
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.sync_bn import BnStatsExchange
    schedule, (B, H, W), attrs, sync = CONFIGS[name]
    dev = torch.device("cuda")
    torch.cuda.synchronize()
    L._ws_cache.clear(); L._state_cache.clear()      # grow-only scratch buffers: their sizes are arguments, and must not depend on what ran before
    args = Namespace(labels={"l0": 0, "l1": 1}, parts={"p0": 0}, fpn_depth=128)            # as _pair() of tests/test_gpu_network.py
    net = Network(args, pretrained=False, raw_output=True).to(dev)
    eng = net._engine
    for k, v in attrs.items():
        setattr(eng, k, list(v) if isinstance(v, list) else v)
    rec = None
    if record:
        rec = eng.lib = _helpers().LaunchRecorder(eng.lib)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, H, W, generator=g).to(dev)
    tail, bits = [], {}
    if schedule.startswith("eval"):
        net.eval()
        net.bf16_inference = schedule == "eval_bf16"
        with torch.no_grad():
            head = net(x)
    else:
        net.train()
        ex = BnStatsExchange.for_network(net, world=1) if sync else None
        if ex is not None:
            ex.log = []
        head, tape = net.forward_train(x, amp=schedule == "train_amp", bn_sync=ex)
        net.backward_from(tape, torch.randn(head.shape, generator=g).to(dev))
        torch.cuda.synchronize()
        bits["flat_grads"] = net.flat_grads
        bits["bn_buffers"] = torch.cat([b.flatten().float() for n, b in net.named_buffers()])
        if ex is not None:
            tail += [f"bn_sync.log {entry}" for entry in ex.log]
        if eng.prof is not None:
            tail += [f"prof {kind!r} {int(flops)} {phase}" for (kind, flops, _, _, phase) in eng.prof]
            tail += [f"prof_shapes {shape}" for shape in eng.prof_shapes]
    torch.cuda.synchronize()
    bits["head"] = head
    digests = {k: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, t in bits.items()}
    return (rec.lines() + tail if record else None), digests


def summary(lines):
    """What the fixture keeps of a trace: the counts, the sha256 of the text, and 16 bits per line to name the first call that differs."""
    return {"calls": len(lines), "symbols": dict(sorted(Counter(line.split("(")[0].split(" ")[0] for line in lines).items())),
            "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest(),
            "line_digests": "".join(hashlib.sha256(line.encode()).hexdigest()[:4] for line in lines)}


def first_difference(lines, want):
    """None if `lines` is the recorded trace, else (index of the first call that differs, that call here or None past the end)."""
    got = summary(lines)
    if got == want:
        return None
    a, b = got["line_digests"], want["line_digests"]
    for i in range(min(len(a), len(b)) // 4):
        if a[4 * i:4 * i + 4] != b[4 * i:4 * i + 4]:
            return i, lines[i]
    n = min(len(a), len(b)) // 4
    return n, (lines[n] if n < len(lines) else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("record", "diff", "digest"))
    ap.add_argument("--root", default=str(HERE)); ap.add_argument("--out", default=None); ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.root).resolve()))
    if a.mode == "digest":
        table = {name: run_config(name, record=False)[1] for name in CONFIGS}
        text = json.dumps(table, indent=1)
        print(text)
        if a.out:
            Path(a.out).write_text(text + "\n")
        return 0
    traces = {name: run_config(name)[0] for name in CONFIGS}
    if a.dump:
        Path(a.dump).mkdir(parents=True, exist_ok=True)
        for name, lines in traces.items():
            (Path(a.dump) / f"{name}.txt").write_text("\n".join(lines) + "\n")
    if a.mode == "record":
        out = Path(a.out or FIXTURE)
        out.write_text(json.dumps({name: summary(lines) for name, lines in traces.items()}, indent=1) + "\n")
        print(f"{out}: {', '.join(f'{n} {len(t)}' for n, t in traces.items())}")
        return 0
    want, bad = json.loads(FIXTURE.read_text()), 0
    for name, lines in traces.items():
        if first_difference(lines, want[name]) is None:
            print(f"{name}: equal ({len(lines)} calls)")
            continue
        bad += 1
        w = want[name]["line_digests"]
        print(f"{name}: {len(lines)} calls here, {want[name]['calls']} recorded")
        for i, line in enumerate(lines):
            if hashlib.sha256(line.encode()).hexdigest()[:4] != w[4 * i:4 * i + 4]:
                print(f"  call {i}: {line}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
