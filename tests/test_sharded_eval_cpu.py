"""Data-parallel evaluation helpers on the CPU (utils/distributed.py): contiguous shards, and the rank-order gathers of
Evaluators, per-image rows and object lists over gloo at world 2 and 3 (ragged and empty shards included)."""
import os
import socket
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("n,world", [(16, 3), (2, 3), (6, 2), (6, 3), (0, 2), (17, 8), (5, 1)])
def test_shard_range_is_contiguous_disjoint_and_covering(n, world):
    from structuredetector_amd.utils.distributed import shard_range
    shards = [shard_range(n, r, world) for r in range(world)]
    assert shards[0][0] == 0 and shards[-1][1] == n
    for (lo, hi), (lo2, _) in zip(shards, shards[1:]):
        assert lo <= hi == lo2                                   # contiguous, in rank order, no overlap
    for r, (lo, hi) in enumerate(shards):
        assert lo == n * r // world
    sizes = [hi - lo for lo, hi in shards]
    assert max(sizes) - min(sizes) <= 1
    assert [i for lo, hi in shards for i in range(lo, hi)] == list(range(n))
    if n < world:
        assert 0 in sizes                                        # empty shards exist and are legal


def test_shard_range_examples():
    from structuredetector_amd.utils.distributed import shard_range
    assert [shard_range(16, r, 3) for r in range(3)] == [(0, 5), (5, 10), (10, 16)]
    assert [shard_range(2, r, 3) for r in range(3)] == [(0, 0), (0, 1), (1, 2)]


def _snapshot(ev):
    out = {}
    for sec in ("anchor_eval", "part_eval", "csi_eval", "classification_eval"):
        evals = getattr(ev, sec)
        out[sec] = [(label, e.tp, e.npos, e.ndet, list(e.acc), list(e.count_errors)) for label, e in evals.items()]
    out["csv"] = ev._csv_kps_str()
    return out


def _worker(rank, world, port, golden_dir, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        from structuredetector_amd.utils.distributed import gather_evaluator, gather_objects, gather_rows, shard_range, world_info
        from tests.test_evaluator_cpu import build
        assert world_info() == (rank, world)
        lo, hi = shard_range(6, rank, world)                     # the 6 scenes of evaluator.npz
        _, ev = build(golden_dir, keep=lambda n: lo <= n < hi)
        merged = gather_evaluator(ev)
        assert merged is not ev
        res = {"ev": _snapshot(merged)}
        # per-image rows: rank r holds images [lo, hi) of a 2-image set at world 3 -> one rank has none
        lo2, hi2 = shard_range(2, rank, world)
        rows = torch.arange(lo2 * 3, hi2 * 3, dtype=torch.float32).reshape(-1, 3)
        res["rows"] = gather_rows(rows).tolist()
        res["rows_dtype"] = str(gather_rows(rows.double()).dtype)
        res["objects"] = gather_objects([f"img_{i}" for i in range(lo, hi)])
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gathers_over_gloo_equal_one_process(golden_dir, world):
    """gather_evaluator over contiguous shards of the evaluator.npz scenes == one Evaluator over all of them: counters, accuracy
    lists IN ORDER and the keypoint CSV; gather_rows / gather_objects return every rank's items in rank (= sample) order on every rank."""
    from tests.test_evaluator_cpu import build
    _, whole = build(golden_dir)
    want = _snapshot(whole)
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), golden_dir, out), nprocs=world, join=True)
    for r in range(world):
        assert out[r]["ev"] == want, f"rank {r}"
        assert out[r]["rows"] == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]
        assert out[r]["rows_dtype"] == "torch.float64"
        assert out[r]["objects"] == [f"img_{i}" for i in range(6)]


def test_world_one_helpers_are_identities(golden_dir, monkeypatch):
    """Without a process group nothing is gathered or initialised: the same objects come back."""
    from structuredetector_amd.utils import distributed as D
    from tests.test_evaluator_cpu import build
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert not dist.is_initialized()
    assert D.init_from_env() is False and not dist.is_initialized()
    assert D.world_info() == (0, 1)
    _, ev = build(golden_dir)
    assert D.gather_evaluator(ev) is ev
    t = torch.ones(4, 3)
    assert D.gather_rows(t) is t
    assert D.gather_objects(["a", "b"]) == ["a", "b"]


def _loss_desc(B=2, M=2, N=1, h=8, w=8, K=4, P=8):
    """A well-formed sd_loss_desc whose pointers are aligned placeholders: every case below is refused before any launch."""
    from structuredetector_amd import _lib as L
    d = L.LossDesc()
    for i, k in enumerate(("anchor_hm", "part_hm", "offsets", "embeddings", "t_anchor_hm", "t_part_hm", "anchor_inds", "part_inds",
                           "anchor_offsets", "part_offsets", "t_embeddings", "anchor_mask", "part_mask")):
        setattr(d, k, 256 * (i + 1))
    d.a_sb, d.a_sc = (M + N + 4) * h * w, h * w
    d.p_sb, d.p_sc = d.a_sb, h * w
    d.o_sb, d.o_sc = d.a_sb, h * w
    d.e_sb, d.e_sc = d.a_sb, h * w
    d.ta_sb, d.ta_sc = M * h * w, h * w
    d.tp_sb, d.tp_sc = N * h * w, h * w
    d.B, d.M, d.N, d.h, d.w, d.K, d.P = B, M, N, h, w, K, P
    d.hm_loss_fn = 0
    d.hm_weight, d.offset_weight, d.embedding_weight = 1.0, 1.0, 1.0
    return d


def test_loss_per_image_c_abi_rejects_bad_arguments_without_touching_the_gpu():
    """sd_loss_fwd_per_image validates like sd_loss_fwd before it launches: null descriptor / output / workspace, a workspace below
    sd_loss_workspace_bytes, bad sizes, an unknown heatmap loss and misaligned heatmaps are refused with SD_ERR_* codes."""
    import ctypes as C
    from structuredetector_amd import _lib as L
    lib = L.lib()
    ws = lib.sd_loss_workspace_bytes(2, 2, 1, 8, 8)
    d = _loss_desc()
    assert lib.sd_loss_fwd_per_image(None, 4096, 8192, ws, 0) == -1 and b"null descriptor" in lib.sd_last_error()
    assert lib.sd_loss_fwd_per_image(C.byref(d), None, 8192, ws, 0) == -1 and b"sd_loss_fwd_per_image" in lib.sd_last_error()
    assert lib.sd_loss_fwd_per_image(C.byref(d), 4096, None, ws, 0) == -1
    assert lib.sd_loss_fwd_per_image(C.byref(d), 4096, 8192, ws - 1, 0) == -2 and b"workspace" in lib.sd_last_error()
    d.part_mask = None
    assert lib.sd_loss_fwd_per_image(C.byref(d), 4096, 8192, ws, 0) == -1 and b"null pointer" in lib.sd_last_error()
    d = _loss_desc()
    d.B = 0
    assert lib.sd_loss_fwd_per_image(C.byref(d), 4096, 8192, ws, 0) == -1 and b"bad sizes" in lib.sd_last_error()
    d = _loss_desc(h=3, w=5)
    assert lib.sd_loss_fwd_per_image(C.byref(d), 4096, 8192, ws, 0) == -1
    d = _loss_desc()
    d.hm_loss_fn = 7
    assert lib.sd_loss_fwd_per_image(C.byref(d), 4096, 8192, ws, 0) == -1 and b"hm_loss_fn" in lib.sd_last_error()
    d = _loss_desc()
    d.t_part_hm = 256 + 4
    assert lib.sd_loss_fwd_per_image(C.byref(d), 4096, 8192, ws, 0) == -3
    d = _loss_desc()
    d.a_sc = 66
    assert lib.sd_loss_fwd_per_image(C.byref(d), 4096, 8192, ws, 0) == -3
