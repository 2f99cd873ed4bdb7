"""Sharded evaluate / detect / validation on the GPU.

  * `sd_loss_fwd_per_image` (Loss.per_image) against B separate B = 1 `sd_loss_fwd` calls, bit for bit;
  * `evaluate` on 2 and 3 ranks with the planted heads of tests/golden/evaluate16.npz: each rank is handed only its contiguous shard and
    the merged Evaluator / CSV equal the reference's on every rank;
  * `Trainer.valid()` on 2 ranks whose BatchNorm buffers differ == one process validating rank 0's model, and each rank keeps its own
    buffers; at world 1 the batched per-image loss gives the bits of the per-image path it replaced;
  * `detect` on 2 ranks writes the files one rank writes.
Multi-rank runs: 2 or 3 processes share the test GPU and talk over gloo (as in tests/test_gpu_dp.py)."""
import json
import os
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

TIMEOUT = timedelta(seconds=300)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the per-image loss
# ---------------------------------------------------------------------------------------------------------------------------------
def _loss_case(B, M, N, fn, seed, size=512):
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    from tests.test_host_cpu import make_args
    dev = torch.device("cuda")
    args = make_args(M, N, 20, 40, device=dev, hm_loss_fn=fn, offset_weight=0.5, embedding_weight=0.25)
    rng = np.random.default_rng(seed)
    n_obj, o_lab, o_xy, o_np, p_kind, p_xy = synthetic_batch(rng, B - 2, size, size, M, N, n_min=1, n_max=30)
    n_obj = np.insert(n_obj, [0, min(5, B - 2)], 0)                  # two images without any object: num_pos == 0, empty masks
    enc = Encode(args)
    tgt = enc.render(enc.plan(size, size, n_obj, o_lab, o_xy, o_np, p_kind, p_xy), dev)
    if B > 3:
        tgt["part_mask"][3] = False                                  # anchors present, every part masked out
    h = size // 4
    head = torch.randn(B, M + N + 4, h, h, device=dev, generator=torch.Generator(dev).manual_seed(seed)) * 3
    return args, head, tgt


def _one_by_one(head, tgt, cfg):
    from structuredetector_amd.model.loss import loss_forward
    keys = ("anchor_hm", "part_hm", "anchor_inds", "part_inds", "anchor_offsets", "part_offsets", "embeddings", "anchor_mask", "part_mask")
    rows = []
    for b in range(head.shape[0]):
        _, _, out8 = loss_forward(head[b:b + 1].contiguous(), {k: tgt[k][b:b + 1] for k in keys}, cfg)
        rows.append(out8)
    return torch.stack(rows)


@pytest.mark.parametrize("fn", ["mse", "focal"])
@pytest.mark.parametrize("B,M,N", [(64, 2, 1), (7, 2, 1), (3, 1, 1), (8, 30, 3)])
def test_loss_per_image_equals_separate_calls_bitwise(fn, B, M, N):
    """Row b of sd_loss_fwd_per_image == sd_loss_fwd on image b alone, every one of the 8 fields, bit for bit: MSE and focal, B up to 64 at
    128^2 maps, images with zero positives and with empty masks, a wide label set (M + N + 4 = 37 > 32), the head as channel views of one
    tensor and as four separate tensors."""
    from structuredetector_amd.model.loss import Loss, loss_config
    args, head, tgt = _loss_case(B, M, N, fn, seed=B * 100 + M)
    cfg = loss_config(args, M, N, 20, 40)
    want = _one_by_one(head, tgt, cfg)
    assert (want[:, 7] == 0).any() and (want[:, 7] > 0).any()                # empty and non-empty part masks
    if fn == "focal":
        assert (want[:, 4] == 0).any() and (want[:, 4] > 0).any()            # num_pos == 0 and > 0 (only the focal loss counts them)
    loss = Loss(args)
    nb = M + N
    views = {"anchor_hm": head[:, :M], "part_hm": head[:, M:nb], "offsets": head[:, nb:nb + 2], "embeddings": head[:, nb + 2:nb + 4]}
    got = loss.per_image(views, tgt)
    assert got.shape == (B, 8) and got.dtype == torch.float32
    assert torch.equal(got, want)
    separate = {k: v.clone() for k, v in views.items()}
    assert torch.equal(loss.per_image(separate, tgt), want)
    # and the batch mean of the old formulation is unaffected: forward over the whole batch still runs sd_loss_fwd
    total = loss(views, tgt)
    assert torch.isfinite(total)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. evaluate on 2 and 3 ranks (planted heads)
# ---------------------------------------------------------------------------------------------------------------------------------
def _evaluate_worker(rank, world, port, tmp, golden_dir, out):
    _init(rank, world, port)
    try:
        from pathlib import Path

        from structuredetector_amd.cli import evaluate
        from structuredetector_amd.data import CropDataset
        from structuredetector_amd.utils.distributed import shard_range
        from tests.helpers import assert_evaluator_equals_golden
        tmp = Path(tmp)
        g = np.load(Path(golden_dir) / "evaluate16.npz")
        heads = np.load(tmp / "heads.npy")
        lo, hi = shard_range(16, rank, world)
        base = ["--valid_dir", str(tmp / "valid"), "-s", "stem", "--labels", str(tmp / "labels.json")]
        host_reader = CropDataset(evaluate.Arguments().parse(base), tmp / "valid")
        res = {}
        for eval_batch in (16, 5, 1):
            seen = []

            class PlantedNetwork(torch.nn.Module):
                def __init__(self, args, *a, **kw):
                    super().__init__()
                    self.dummy = torch.nn.Parameter(torch.zeros(1))

                def forward(self, x):
                    assert tuple(x.shape[1:]) == (3, 512, 512) and x.shape[0] <= eval_batch and x.is_cuda
                    i = lo + len(seen)
                    seen.extend(x.cpu())
                    h = torch.from_numpy(heads[i:i + x.shape[0]]).to(x.device)
                    return {"anchor_hm": h[:, :2], "part_hm": h[:, 2:3], "offsets": h[:, 3:5], "embeddings": h[:, 5:7]}

            evaluate.Network = PlantedNetwork
            csv = tmp / f"kps_w{world}_b{eval_batch}.csv"
            ev = evaluate.main(base + ["--eval_batch", str(eval_batch), "--save_csv_eval", str(csv)])
            assert len(seen) == hi - lo, f"rank {rank} was handed {len(seen)} images, its shard has {hi - lo}"
            for j, img in enumerate(seen):
                assert torch.equal(img, host_reader[lo + j][0]), f"rank {rank}, image {lo + j}: differs from the PIL chain"
            assert_evaluator_equals_golden(ev, g)
            res[eval_batch] = True
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_evaluate_sharded_on_16_png_json_samples_vs_reference(golden_dir, tmp_path, world):
    """`evaluate` on `world` ranks over the 16-sample directory of test_evaluate_on_16_png_json_samples_vs_reference, at --eval_batch
    16 / 5 / 1: each rank's network sees exactly its contiguous shard (bit-identical to the PIL chain), the merged Evaluator equals the
    reference's goldens on every rank, and the CSV rank 0 writes is byte-identical to the reference's."""
    from tests.helpers import write_evaluate16_dir
    g = np.load(golden_dir / "evaluate16.npz")
    np.save(tmp_path / "heads.npy", np.stack(write_evaluate16_dir(g, tmp_path / "valid")))
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    out = mp.Manager().dict()
    mp.spawn(_evaluate_worker, args=(world, _free_port(), str(tmp_path), str(golden_dir), out), nprocs=world, join=True)
    for r in range(world):
        assert out[r] == {16: True, 5: True, 1: True}
    for b in (16, 5, 1):
        assert (tmp_path / f"kps_w{world}_b{b}.csv").read_text() == str(g["csv"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. / 5. Trainer.valid()
# ---------------------------------------------------------------------------------------------------------------------------------
def _valid_argv(tmp, mode):
    base = ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp / "labels.json"), "-b", "4"]
    if mode == "synthetic":
        return base + ["--synthetic", "16", "--eval_batch", "3"]
    return base + ["--train_dir", str(tmp / "valid"), "--valid_dir", str(tmp / "valid"), "--eval_batch", "4"]


def _perturb_buffers(net, rank):
    """Rank-dependent BatchNorm running statistics (they are rank-local in training)."""
    g = torch.Generator().manual_seed(1000 + rank)
    with torch.no_grad():
        for name, b in net.named_buffers():
            if name.endswith("running_mean"):
                b.add_((torch.rand(b.shape, generator=g) * 0.2 - 0.1).to(b.device))
            elif name.endswith("running_var"):
                b.mul_((1.0 + torch.rand(b.shape, generator=g) * 0.5).to(b.device))


def _evaluator_snapshot(ev):
    out = {}
    for sec in ("anchor_eval", "part_eval", "csi_eval", "classification_eval"):
        out[sec] = [(label, e.tp, e.npos, e.ndet, list(e.acc)) for label, e in getattr(ev, sec).items()]
    out["csv"] = ev._csv_kps_str()
    return out


def _valid_result(tr, stats):
    return {"stats": (stats.hm_loss, stats.offset_loss, stats.embedding_loss), "ev": _evaluator_snapshot(tr.evaluator),
            "best": tuple(getattr(tr, k) for k in ("best_loss", "best_csi", "best_classif", "best_kp_reg"))}


def _valid_worker(rank, world, port, tmp, out):
    _init(rank, world, port)
    try:
        from pathlib import Path

        from structuredetector_amd.model.trainer import Trainer
        from structuredetector_amd.utils.args import Arguments
        tmp = Path(tmp)
        res = {}
        for mode in ("synthetic", "directory"):
            torch.manual_seed(5)
            tr = Trainer(Arguments().parse(_valid_argv(tmp, mode)))
            assert tr.step.world == world
            _perturb_buffers(tr.net, rank)
            own = {k: v.detach().clone() for k, v in tr.net.named_buffers()}
            tr.save_dir = tmp / f"dp_{mode}"
            if rank == 0:
                torch.save({k: v.detach().cpu() for k, v in tr.net.state_dict().items()}, tmp / f"rank0_{mode}.pth")
            dist.barrier()
            stats = tr.valid()
            after = dict(tr.net.named_buffers())
            res[mode] = _valid_result(tr, stats)
            res[mode]["own_buffers_back"] = all(torch.equal(after[k], v) for k, v in own.items())
            res[mode]["training_mode"] = tr.net.training and not tr.net._folded
        out[rank] = res
    finally:
        dist.destroy_process_group()


def _old_per_image_stats(tr):
    """The validation loss as computed before the batched path: one Encode.batch + one Loss call per image on that image's slice of the
    head, then the float64 mean over images."""
    from structuredetector_amd.model.loss import LossStats
    from structuredetector_amd.model.predictor import batched_outputs
    a = tr.args
    tr.net.eval()
    if tr.valid_set is not None:
        samples = batched_outputs(tr.net, tr.decoder, tr.valid_set, a, keep_output=True)
    else:
        from structuredetector_amd.data.synthetic import synthetic_samples

        def samples_gen():
            for image, annotation in synthetic_samples(a, 16, seed=20261003):
                with torch.no_grad():
                    yield None, annotation, None, tr.net(image[None].to(a.device))
        samples = samples_gen()
    per_image = []
    for _, annotation, _, output in samples:
        with torch.no_grad():
            target = tr.encode.batch((a.width, a.height), [annotation], a.device)
            tr.loss(output, target)
        per_image.append(torch.stack([tr.loss.stats.hm_loss, tr.loss.stats.offset_loss, tr.loss.stats.embedding_loss]))
    tr.net.train()
    stats = LossStats(*(torch.stack(per_image).double().sum(0).tolist()))
    stats /= len(per_image)
    return stats


def test_valid_two_ranks_scores_rank0_model_and_restores_buffers(golden_dir, tmp_path, monkeypatch):
    """Trainer.valid() on 2 ranks whose BatchNorm buffers differ, synthetic and directory validation (--eval_batch 4 divides the two
    8-image shards, so the batches are the one-process batches): the merged loss statistics, Evaluator and best-so-far values equal a
    one-process valid() of rank 0's model bit for bit, on BOTH ranks; each rank has its own buffers back afterwards; the model_best_*.pth
    rank 0 writes are byte-identical to the one-process run's.  The one-process valid() also equals the per-image loss path it replaces."""
    from structuredetector_amd.model.trainer import Trainer
    from structuredetector_amd.utils.args import Arguments
    from tests.helpers import write_evaluate16_dir
    g = np.load(golden_dir / "evaluate16.npz")
    write_evaluate16_dir(g, tmp_path / "valid")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    monkeypatch.chdir(tmp_path)
    out = mp.Manager().dict()
    mp.spawn(_valid_worker, args=(2, _free_port(), str(tmp_path), out), nprocs=2, join=True)
    for mode in ("synthetic", "directory"):
        tr = Trainer(Arguments().parse(_valid_argv(tmp_path, mode)))
        assert tr.step.world == 1
        tr.net.load_state_dict(torch.load(tmp_path / f"rank0_{mode}.pth", map_location="cpu", weights_only=True))
        tr.save_dir = tmp_path / f"single_{mode}"
        stats = tr.valid()
        want = _valid_result(tr, stats)
        for r in range(2):
            got = out[r][mode]
            assert got["own_buffers_back"] and got["training_mode"], (mode, r)
            assert got["stats"] == want["stats"], (mode, r, got["stats"], want["stats"])
            assert got["ev"] == want["ev"], (mode, r)
            assert got["best"] == want["best"], (mode, r)
        single = sorted(p.name for p in (tmp_path / f"single_{mode}").glob("model_best_*.pth"))
        assert single and single == sorted(p.name for p in (tmp_path / f"dp_{mode}").glob("model_best_*.pth"))
        for name in single:
            assert (tmp_path / f"single_{mode}" / name).read_bytes() == (tmp_path / f"dp_{mode}" / name).read_bytes(), (mode, name)
        # 5. world 1: the batched per-image loss == the old one-call-per-image path, bit for bit
        old = _old_per_image_stats(tr)
        assert (stats.hm_loss, stats.offset_loss, stats.embedding_loss) == (old.hm_loss, old.offset_loss, old.embedding_loss), mode


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. detect on 2 ranks
# ---------------------------------------------------------------------------------------------------------------------------------
def _detect_argv(tmp):
    return ["--valid_dir", str(tmp / "jpg"), "-W", "256", "-H", "256", "-s", "stem", "--labels", str(tmp / "labels.json"),
            "--eval_batch", "3", "-o", str(tmp / "seeded.pth"), "--conf_threshold", "0.05"]


def _detect_worker(rank, world, port, tmp, out):
    _init(rank, world, port)
    try:
        from pathlib import Path

        from structuredetector_amd.cli import detect
        tmp = Path(tmp)
        os.chdir(tmp / "dp")
        written = detect.main(_detect_argv(tmp))
        out[rank] = [str(p) for p in written]
    finally:
        dist.destroy_process_group()


def test_detect_two_ranks_writes_the_files_of_one_rank(golden_dir, tmp_path, monkeypatch):
    """`detect` on 2 ranks: together they write the same set of files, with the same bytes, as one rank, and main() returns the whole
    list in directory order on both ranks."""
    from PIL import Image

    from oracle import sdnet_oracle as O
    from structuredetector_amd.cli import detect
    from tests.helpers import write_evaluate16_dir
    g = np.load(golden_dir / "evaluate16.npz")
    write_evaluate16_dir(g, tmp_path / "png")
    (tmp_path / "jpg").mkdir()
    for i in range(7):                                                 # 7 images: shards of 3 and 4, a ragged batch on each rank
        Image.open(tmp_path / "png" / f"img_{i:02d}.png").convert("RGB").save(tmp_path / "jpg" / f"img_{i:02d}.jpg", quality=90)
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    torch.save(O.build_reference_network(2, 1, seed=16).state_dict(), tmp_path / "seeded.pth")
    (tmp_path / "dp").mkdir()
    (tmp_path / "single").mkdir()
    out = mp.Manager().dict()
    mp.spawn(_detect_worker, args=(2, _free_port(), str(tmp_path), out), nprocs=2, join=True)
    monkeypatch.chdir(tmp_path / "single")
    written = [str(p) for p in detect.main(_detect_argv(tmp_path))]
    assert len(written) == 7 and out[0] == out[1] == written
    single = sorted(p.name for p in (tmp_path / "single" / "predictions").iterdir())
    dp = sorted(p.name for p in (tmp_path / "dp" / "predictions").iterdir())
    assert len(single) == 14 and single == dp
    for name in single:
        assert (tmp_path / "single" / "predictions" / name).read_bytes() == (tmp_path / "dp" / "predictions" / name).read_bytes(), name
