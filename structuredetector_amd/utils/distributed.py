"""Data-parallel evaluation: contiguous shards, rank-order gathers and the process-group setup of the CLIs.

Evaluate, detect and the trainer's validation pass split their images into CONTIGUOUS blocks, one per rank
(`shard_range`), and merge per-rank results in rank order, which gives dataset order back.  Accuracy lists,
`avg_acc`, the keypoint CSV and the float64 loss sums depend on that order down to the last bit; strided
shards would reorder them.  A rank whose shard is empty (n < world) still takes part in every collective.
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist


def world_info(group=None):
    """(rank, world) of the initialised process group, (0, 1) without one."""
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def shard_range(n, rank, world):
    """[lo, hi) of rank's contiguous block of n items: lo = n * rank // world.  Blocks are disjoint, cover range(n) in
    rank order and differ in length by at most one; some are empty when n < world."""
    return n * rank // world, n * (rank + 1) // world


def _gather_objects(obj, group):
    out = [None] * dist.get_world_size(group)
    dist.all_gather_object(out, obj, group=group)
    return out


def gather_evaluator(evaluator, group=None):
    """Every rank's four Evaluations, merged in rank order into a fresh Evaluator (`Evaluator.merge`); every rank returns the same
    merged object.  Without a process group (or at world 1) the evaluator itself is returned."""
    from ..model.evaluator import Evaluator
    _, world = world_info(group)
    if world == 1:
        return evaluator
    parts = _gather_objects((evaluator.anchor_eval, evaluator.part_eval, evaluator.csi_eval, evaluator.classification_eval), group)
    merged = Evaluator(evaluator.args)
    for anchor, part, csi, classif in parts:
        other = Evaluator.__new__(Evaluator)
        other.anchor_eval, other.part_eval, other.csi_eval, other.classification_eval = anchor, part, csi, classif
        merged.merge(other)
    return merged


def gather_pr_curve(curve, group=None):
    """Every rank's PrCurve tables, merged in rank order into a fresh PrCurve (`PrCurve.merge`); every rank returns the same merged
    object.  Without a process group (or at world 1) the curve itself is returned."""
    from ..model.pr_curve import PrCurve
    _, world = world_info(group)
    if world == 1:
        return curve
    parts = _gather_objects((curve.tables, curve.images, curve.redone), group)
    merged = PrCurve(curve.args, curve.thresholds)
    for tables, images, redone in parts:
        other = PrCurve(curve.args, curve.thresholds)
        other.tables, other.images, other.redone = tables, images, redone
        merged.merge(other)
    return merged


def gather_objects(items, group=None):
    """Every rank's list concatenated in rank order (on every rank); `items` itself at world 1."""
    _, world = world_info(group)
    if world == 1:
        return list(items)
    return [x for part in _gather_objects(list(items), group) for x in part]


def gather_rows(tensor, group=None):
    """All-gather of variable-length per-image rows: every rank's (n_r, k) tensor, concatenated in rank order, on the device of
    `tensor` (exact copies of the values).  Ranks with no rows pass an empty (0, k) tensor.  `tensor` itself at world 1."""
    _, world = world_info(group)
    if world == 1:
        return tensor
    dev = tensor.device
    comm = dev if dist.get_backend(group) == "nccl" else torch.device("cpu")
    rows = tensor.detach().to(comm).contiguous()
    counts = [torch.zeros(1, dtype=torch.int64, device=comm) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([rows.shape[0]], dtype=torch.int64, device=comm), group=group)
    counts = [int(c.item()) for c in counts]
    longest = max(counts)
    if longest == 0:
        return tensor
    padded = torch.zeros((longest,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=comm)
    padded[:rows.shape[0]] = rows
    bufs = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(bufs, padded, group=group)
    return torch.cat([b[:c] for b, c in zip(bufs, counts)]).to(dev)


def init_from_env():
    """Process-group setup for the evaluate / detect CLIs.  An initialised group is used as it is.  Otherwise, under a launcher
    (WORLD_SIZE > 1, e.g. `python -m torch.distributed.run --nproc-per-node N`), the device is set from LOCAL_RANK and an nccl
    group is initialised, as `cli/train.py` does.  At world 1 nothing happens.  Returns True when this call created the group
    (the caller then destroys it)."""
    if dist.is_available() and dist.is_initialized():
        return False
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
        return True
    return False
