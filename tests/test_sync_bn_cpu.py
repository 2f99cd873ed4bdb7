"""Synchronized BatchNorm without a GPU: the `--sync_bn` flag and its way into `TrainStep`, the statistics exchange over CPU gloo
(every rank gets the same fp64 bits, the fp64 sum), and the argument checks of the split-finish C-ABI entry points."""
import ctypes as C
import inspect
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

SD_ERR_INVALID, SD_ERR_ALIGN = -1, -3


def test_flag_defaults_off_and_reaches_train_step():
    from structuredetector_amd.model.trainer import TrainStep, train_step_kwargs
    from structuredetector_amd.utils.args import Arguments
    p = Arguments().parser
    off, on = p.parse_args([]), p.parse_args(["--sync_bn", "-l", "0.01"])
    assert off.sync_bn is False and on.sync_bn is True
    assert train_step_kwargs(off) == dict(lr=1e-3, sync_bn=False)
    assert train_step_kwargs(on) == dict(lr=0.01, sync_bn=True)
    assert inspect.signature(TrainStep).parameters["sync_bn"].default is False
    assert set(train_step_kwargs(on)) <= set(inspect.signature(TrainStep).parameters)
    help_text = " ".join(p.format_help().split())
    assert "--sync_bn Synchronized BatchNorm" in help_text


def test_pack_and_unpack_sums():
    from structuredetector_amd.model.sync_bn import pack_sums, unpack_sums
    v = pack_sums([1.0, 2.0], [3.0, 4.0], 10)
    assert v.dtype == torch.float64 and v.tolist() == [1.0, 2.0, 3.0, 4.0, 10.0]
    s0, s1, n = unpack_sums(v)
    assert s0.tolist() == [1.0, 2.0] and s1.tolist() == [3.0, 4.0] and n == 10.0
    with pytest.raises(ValueError):
        unpack_sums(torch.zeros(4, dtype=torch.float64))


def test_arena_slots_and_bounds():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model.sync_bn import BnStatsExchange
    ex = BnStatsExchange([4, 8], "cpu", world=1)
    assert ex.arena.numel() == 2 * (9 + 17) and ex.arena.dtype == torch.float64
    ex.begin("fwd")
    a, b = ex.take(4), ex.take(8)
    assert a.numel() == 9 and b.numel() == 17 and b.data_ptr() == a.data_ptr() + 9 * 8
    with pytest.raises(L.SdError):
        ex.take(4)
    ex.begin("bwd")
    assert ex.take(4).data_ptr() == ex.arena.data_ptr() + 26 * 8      # backward slots: the second half
    a.fill_(3.0)
    ex.reduce(a)                                                       # one rank: no collective, nothing changes
    assert a.tolist() == [3.0] * 9


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _exchange_worker(rank, world, port, outdir):
    from datetime import timedelta
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    try:
        from structuredetector_amd.model.sync_bn import BnStatsExchange, pack_sums
        channels = [64, 128, 512]
        ex = BnStatsExchange(channels, "cpu")
        assert ex.world == world
        g = torch.Generator().manual_seed(1000 + rank)
        sent, got = [], []
        for direction in ("fwd", "bwd"):
            ex.begin(direction)
            for c in channels:
                slot = ex.take(c)
                # random fp64 sums (any bits) and a per-rank element count (ranks with different batch sizes)
                v = pack_sums(torch.randn(c, generator=g, dtype=torch.float64) * 1e3, torch.rand(c, generator=g, dtype=torch.float64) * 1e6,
                              (rank + 1) * 4096)
                slot.copy_(v)
                sent.append(v.clone())
                ex.reduce(slot)
                got.append(slot.clone())
        torch.save(dict(sent=sent, got=got), os.path.join(outdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_exchange_over_gloo_gives_every_rank_the_same_fp64_sum(world, tmp_path):
    mp.spawn(_exchange_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    for k in range(len(res[0]["got"])):
        got = [r["got"][k] for r in res]
        for g in got[1:]:
            assert torch.equal(g.view(torch.int64), got[0].view(torch.int64))       # the same bits on every rank
        exact = torch.stack([r["sent"][k] for r in res])
        assert got[0][-1].item() == sum(4096 * (r + 1) for r in range(world))        # the count is summed exactly
        if world == 2:
            assert torch.equal(got[0], exact[0] + exact[1])                          # two addends: one rounding, any order
        else:                                                                        # three: the fp64 sum in one of its association orders
            a, b, c = exact
            assert bool((((a + b) + c == got[0]) | ((a + c) + b == got[0]) | ((b + c) + a == got[0])).all())


def test_split_finish_entry_points_reject_bad_arguments():
    """Every split-finish export validates before it launches (no GPU is touched): null pointers, a bad channel count, a bad row
    count and a misaligned fp64 buffer come back as SD_ERR_INVALID / SD_ERR_ALIGN with a message naming the entry point."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    big = 1 << 30

    def rejects(rc, name, code=SD_ERR_INVALID, needle=None):
        msg = lib.sd_last_error()
        assert rc == code, (name, rc, msg)
        assert name.encode() in msg, (name, msg)
        if needle:
            assert needle.encode() in msg, (name, msg)

    rejects(lib.sd_bn_stats_sums(0, 4, 100, 64, 16, 0, 0), "sd_bn_stats_sums", needle="null")
    rejects(lib.sd_bn_stats_sums(16, 0, 100, 64, 16, 0, 0), "sd_bn_stats_sums", needle="rows")
    rejects(lib.sd_bn_stats_sums(16, 4, 100, 6, 16, 0, 0), "sd_bn_stats_sums", needle="C in")
    rejects(lib.sd_bn_stats_sums(16, 4, 100, 64, 20, 0, 0), "sd_bn_stats_sums", SD_ERR_ALIGN)
    rejects(lib.sd_bn_stats_from_sums(0, 64, C.c_float(1e-5), C.c_float(0.1), 0, 0, 16, 16, 0), "sd_bn_stats_from_sums")
    rejects(lib.sd_bn_stats_from_sums(16, 6, C.c_float(1e-5), C.c_float(0.1), 0, 0, 16, 16, 0), "sd_bn_stats_from_sums", needle="C in")
    rejects(lib.sd_bn_stats_from_sums(16, 64, C.c_float(1e-5), C.c_float(0.1), 16, 0, 16, 16, 0), "sd_bn_stats_from_sums")   # one running buffer
    rejects(lib.sd_bn_bwd_sums(16, 0, 100, 64, 16, 16, 0, 16, 0, 0), "sd_bn_bwd_sums", needle="rows")
    rejects(lib.sd_bn_bwd_sums(16, 4, 100, 64, 0, 16, 0, 16, 0, 0), "sd_bn_bwd_sums")
    rejects(lib.sd_bn_bwd_sums(16, 4, 100, 2000, 16, 16, 0, 16, 0, 0), "sd_bn_bwd_sums", needle="C in")
    rejects(lib.sd_bn_bwd_means_from_sums(16, 64, 0, 0), "sd_bn_bwd_means_from_sums")
    rejects(lib.sd_bn_bwd_means_from_sums(16, 0, 16, 0), "sd_bn_bwd_means_from_sums", needle="C in")
    rejects(lib.sd_bn_bwd_means_from_sums(12, 64, 16, 0), "sd_bn_bwd_means_from_sums", SD_ERR_ALIGN)
    rejects(lib.sd_bn_train_sums(16, 100, 64, 0, 16, big, 0), "sd_bn_train_sums")
    rejects(lib.sd_bn_train_sums_bf16(16, 0, 64, 16, 16, big, 0), "sd_bn_train_sums_bf16", needle="M > 0")
    rejects(lib.sd_bn_bwd_reduce(16, 16, 0, 2, 100, 64, 16, 16, 16, 16, 16, 16, 0, 0, 16, big, 0), "sd_bn_bwd_reduce")
    rejects(lib.sd_bn_bwd_reduce(16, 16, 0, 5, 100, 64, 16, 16, 16, 16, 16, 16, 0, 16, 16, big, 0), "sd_bn_bwd_reduce", needle="relu")
    rejects(lib.sd_bn_bwd_reduce_bf16(16, 16, 0, 1, 100, 64, 16, 16, 16, 16, 16, 16, 0, 16, 16, big, 0), "sd_bn_bwd_reduce_bf16")  # relu 1 needs y
    rejects(lib.sd_bn_bwd_apply_bf16(16, 16, 0, 2, 100, 64, 16, 16, 16, 16, 0, 16, 0, 0), "sd_bn_bwd_apply_bf16")
    rejects(lib.sd_maxpool_bn_relu_bwd_reduce(16, 16, 16, 2, 8, 8, 64, 16, 16, 16, 16, 16, 16, 0, 0, 16, big, 0), "sd_maxpool_bn_relu_bwd_reduce")
    rejects(lib.sd_maxpool_bn_relu_bwd_reduce_bf16(16, 16, 16, 2, 7, 8, 64, 16, 16, 16, 16, 16, 16, 0, 16, 16, big, 0),
            "sd_maxpool_bn_relu_bwd_reduce_bf16", needle="even")
    rejects(lib.sd_maxpool_bn_relu_bwd_apply(16, 16, 16, 2, 8, 8, 64, 16, 16, 16, 16, 0, 16, 0), "sd_maxpool_bn_relu_bwd_apply")
    rejects(lib.sd_maxpool_bn_relu_bwd_apply_bf16(16, 16, 16, 2, 8, 8, 6, 16, 16, 16, 16, 16, 16, 0), "sd_maxpool_bn_relu_bwd_apply_bf16",
            needle="C in")
    rejects(lib.sd_maxpool_bn_relu_bwd_apply_bf16_dx16(16, 16, 16, 2, 8, 8, 64, 16, 16, 16, 16, 16, 0, 0), "sd_maxpool_bn_relu_bwd_apply_bf16_dx16")
    d = L.ConvDesc()
    d.B, d.Hi, d.Wi, d.Cin, d.Cout, d.R, d.S, d.stride, d.pad, d.Ho, d.Wo = 2, 16, 16, 64, 64, 3, 3, 1, 1, 16, 16
    rejects(lib.sd_conv2d_fwd_bn_sums(16, 16, 16, C.byref(d), 0, 16, big, 0), "sd_conv2d_fwd_bn_sums")
    rejects(lib.sd_conv2d_fwd_bn_sums(16, 16, 16, C.byref(d), 20, 16, big, 0), "sd_conv2d_fwd_bn_sums", SD_ERR_ALIGN)
    rejects(lib.sd_conv2d_fwd_bf16_bn_sums(16, 16, 16, C.byref(d), 0, 16, big, 0), "sd_conv2d_fwd_bf16_bn_sums")
    rejects(lib.sd_conv2d_dgrad_bn_reduce_sums(16, 16, 16, C.byref(d), 0, 16, 0, 2, 16, 16, 16, 16, 16, 16, 0, 0, 16, big, 0),
            "sd_conv2d_dgrad_bn_reduce_sums")
    for stem in ("sd_conv2d_stem_fwd_bn_sums", "sd_conv2d_stem_fwd_bn_sums_bf16mm", "sd_conv2d_stem_fwd_bn_sums_bf16"):
        rejects(getattr(lib, stem)(16, 16, 16, C.byref(d), 16, 16, big, 0), stem, needle="7x7")             # not the stem's geometry
        rejects(getattr(lib, stem)(16, 16, 16, C.byref(d), 0, 16, big, 0), stem)
    # the host query of the fused statistics: rows of partials, 0 for the two-pass form, -1 for an unsupported geometry
    assert lib.sd_conv2d_fwd_bn_stats_rows(None, 0) == -1
    assert lib.sd_conv2d_fwd_bn_stats_rows(C.byref(d), 0) >= 0
    d.Cout = 48
    assert lib.sd_conv2d_fwd_bn_stats_rows(C.byref(d), 0) == -1
