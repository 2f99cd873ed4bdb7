"""Device-resident decoded-image cache (`--cache_images`, data/image_cache.py) on the GPU: the pointer-table entry points
(sd_preprocess_images_list[_jitter]) against the packed ones bit for bit, the cached feed against the host feed (images, annotations,
decode counts), the budget / invalidation / annotation isolation rules, and `train` end to end with and without the cache."""
import json
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _arena_with(imgs, rng):
    """The images copied into one device arena at odd byte offsets; returns (arena, device addresses)."""
    offs, o = [], 0
    for k, im in enumerate(imgs):
        o = (o + 15) // 16 * 16 + 16 + 4 * k + 1 + 2 * int(rng.integers(0, 2))  # odd starts, each at its own offset mod 16
        offs.append(o)
        o += im.nbytes
    arena = torch.zeros(o + 64, dtype=torch.uint8, device=DEV)
    for im, off in zip(imgs, offs):
        arena[off:off + im.nbytes].copy_(torch.from_numpy(im).reshape(-1).to(DEV))
    return arena, [arena.data_ptr() + off for off in offs]


@pytest.mark.parametrize("hin,win,sizes", [(37, 53, [(96, 64), (32, 16)]), (480, 640, [(320, 256), (800, 608)]),
                                           (2048, 2448, [(512, 512), (2560, 2112)])])
def test_list_entry_points_equal_the_packed_ones_bitwise(hin, win, sizes):
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    from structuredetector_amd.data.augment import jitter_words
    rng = np.random.default_rng(hin + win)
    n = 3
    imgs = [rng.integers(0, 256, (hin, win, 3), dtype=np.uint8) for _ in range(n)]
    arena, addrs = _arena_with(imgs, rng)
    assert len({a % 16 for a in addrs}) == n and all(a % 2 == 1 for a in addrs)
    order = [2, 0, 2, 1, 0, 1]                                             # shuffled, with duplicates
    table = torch.tensor([addrs[t] for t in order], dtype=torch.int64, device=DEV)
    packed = torch.from_numpy(np.stack([imgs[t] for t in order])).to(DEV)
    B = len(order)
    flips = [k % 4 for k in range(B)]                                      # all four flip codes
    jit = [jitter_words(list(rng.permutation(4)), *rng.uniform(0.75, 1.25, 2), rng.uniform(0.85, 1.15), rng.uniform(-0.05, 0.05))
           for _ in range(B)]
    jitter = ([w for w, _ in jit], [f for _, f in jit])
    assert len({w & 0xFF for w in jitter[0]}) > 1                          # several op orders
    for size in sizes:
        for f in (None, flips):
            want = preprocess_images(packed, size, f)
            got = preprocess_image_list(table, hin, win, size, f)
            assert got.shape == (B, 3, size[1], size[0]) and torch.equal(got, want), (size, f)
        want = preprocess_images(packed, size, flips, jitter=jitter)
        got = preprocess_image_list(table, hin, win, size, flips, jitter=jitter)
        assert torch.equal(got, want), (size, "jitter")
    torch.cuda.synchronize()
    del arena


def _counting(ds_cls):
    class Counting(ds_cls):
        decodes = 0

        def __getitem__(self, index):
            type(self).decodes += 1
            return super().__getitem__(index)
    return Counting


def _ann_rows(ann):
    return (str(ann.image_path), tuple(ann.img_size) if ann.img_size is not None else None,
            [(o.name, o.anchor.kind, o.anchor.x, o.anchor.y, [(p.kind, p.x, p.y) for p in o.parts]) for o in ann.objects])


def _setup(golden_dir, tmp_path, width=128, height=96):
    from structuredetector_amd.data import CropDataset
    from tests.helpers import EVAL16_LABELS, EVAL16_PARTS, write_evaluate16_dir
    g = np.load(golden_dir / "evaluate16.npz")
    write_evaluate16_dir(g, tmp_path / "train")
    args = Namespace(labels=EVAL16_LABELS, parts=EVAL16_PARTS, width=width, height=height, anchor_name="stem", no_augmentation=False,
                     device=torch.device(DEV, torch.cuda.current_device()))
    return args, _counting(CropDataset)(args, tmp_path / "train", raw=True)


def _pass_order(p, n):
    order = np.random.default_rng(p).permutation(n)
    return [order[i:i + 5] for i in range(0, 15, 5)]


def _passes(ds, args, cache, passes=3, seed=11):
    """`passes` epochs of BatchFeeder + TrainAugmentation (seeded), shuffled batches of mixed sizes: per pass, the preprocessed tensors and
    the augmented annotations."""
    from structuredetector_amd.data import BatchFeeder, TrainAugmentation
    torch.manual_seed(seed)
    aug = TrainAugmentation(args)
    out = []
    for p in range(passes):
        batches = _pass_order(p, len(ds))
        got = []
        for batch in BatchFeeder(ds, batches, DEV, workers=3, depth=2, cache=cache):
            images, anns = aug(batch, batch.annotations)
            got.append((images.cpu(), [_ann_rows(a) for a in anns]))
        out.append(got)
        aug.trigger_random_resize()
    return out


def _assert_same(a, b):
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        assert len(pa) == len(pb)
        for (ia, aa), (ib, ab) in zip(pa, pb):
            assert torch.equal(ia, ib)
            assert aa == ab


def test_cached_feed_equals_the_host_feed_and_decodes_nothing_after_prefill(golden_dir, tmp_path):
    from structuredetector_amd.data import DeviceImageCache, ImageList
    args, ds = _setup(golden_dir, tmp_path)
    want = _passes(ds, args, None)
    assert type(ds).decodes == 45
    type(ds).decodes = 0
    cache = DeviceImageCache(1 << 30, DEV)
    assert cache.prefill(ds, workers=4) == 16 and type(ds).decodes == 16 and len(cache) == 16
    assert cache.prefill(ds, workers=4) == 0 and type(ds).decodes == 16            # everything cached already
    got = _passes(ds, args, cache)
    assert type(ds).decodes == 16                                                  # passes 1-3: no decode at all
    _assert_same(got, want)
    st = cache.stats()
    assert st["hits"] == 45 and st["misses"] == 0 and st["refused"] == 0 and st["images"] == 16
    assert st["bytes_used"] == sum(int(ds[j][0].numel()) for j in range(16)) and st["prefill_seconds"] > 0
    # the batches carry pointer tables, not packed tensors
    from structuredetector_amd.data import BatchFeeder
    b = next(iter(BatchFeeder(ds, [[0, 1, 2]], DEV, workers=2, cache=cache)))
    assert all(isinstance(v, ImageList) and v.pointers.dtype == torch.int64 for _, v in b.groups.values())


def test_cache_fills_on_misses_and_a_partial_budget_gives_the_same_batches(golden_dir, tmp_path):
    """No prefill: pass 1 decodes, inserts what fits; a budget below the set: partial hits, the rest decoded every pass, same bytes."""
    from structuredetector_amd.data import DeviceImageCache
    args, ds = _setup(golden_dir, tmp_path)
    want = _passes(ds, args, None)
    total = sum(int(ds[j][0].numel()) for j in range(16))
    seen = len({int(j) for p in range(3) for b in _pass_order(p, 16) for j in b})     # distinct samples the three passes read
    for budget in (1 << 30, 6_000_000):
        type(ds).decodes = 0
        cache = DeviceImageCache(budget, DEV, arena_bytes=4_000_000)
        got = _passes(ds, args, cache)
        _assert_same(got, want)
        st = cache.stats()
        assert st["hits"] + st["misses"] == 45 and st["misses"] == type(ds).decodes
        assert st["images"] + st["refused"] == seen
        assert st["bytes_used"] <= st["bytes_allocated"] <= budget
        if budget < total:
            assert st["refused"] > 0 and st["hits"] > 0 and st["images"] > 0
        else:
            assert st["refused"] == 0 and st["misses"] == seen                     # a pass looks its batches up before it inserts


def test_cache_invalidation_and_annotation_isolation(golden_dir, tmp_path):
    from PIL import Image

    from structuredetector_amd.data import BatchFeeder, DeviceImageCache, TrainAugmentation, preprocess_image_list, preprocess_images
    args, ds = _setup(golden_dir, tmp_path)
    cache = DeviceImageCache(1 << 30, DEV)
    cache.prefill(ds, workers=4)
    fresh = [_ann_rows(ds[j][1]) for j in range(16)]
    torch.manual_seed(3)
    aug = TrainAugmentation(args)
    batches = [list(range(0, 8)), list(range(8, 16))]
    for _ in range(2):                                                              # epoch 1 mutates its annotations in place
        for batch, idx in zip(BatchFeeder(ds, batches, DEV, workers=2, cache=cache), batches):
            assert [_ann_rows(a) for a in batch.annotations] == [fresh[j] for j in idx]   # every epoch: a fresh parse
            aug(batch, batch.annotations)
    # rewriting an image (new size, then same bytes with a new mtime) re-decodes it; the rest stay hits
    path = tmp_path / "train" / "img_05.png"
    Image.open(path).resize((200, 150)).save(path)
    type(ds).decodes = 0
    for batch in BatchFeeder(ds, [[5, 6]], DEV, workers=2, cache=cache):
        assert (150, 200) in batch.groups and type(ds).decodes == 1
        pos, lst = batch.groups[(150, 200)]
        got = torch.from_numpy(np.asarray(Image.open(path).convert("RGB")).copy()).to(DEV)
        assert torch.equal(preprocess_image_list(lst.pointers, 150, 200, (64, 64)), preprocess_images(got[None], (64, 64)))
        assert batch.annotations[pos[0]].img_size == (200, 150)
    for batch in BatchFeeder(ds, [[5]], DEV, workers=2, cache=cache):
        pass
    assert type(ds).decodes == 1                                                    # cached again after the re-decode
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    for batch in BatchFeeder(ds, [[5]], DEV, workers=2, cache=cache):
        pass
    assert type(ds).decodes == 2


def _train_run(tmp_path, name, extra, monkeypatch, capsys):
    from structuredetector_amd.cli import train
    from structuredetector_amd.model import trainer as T
    run = tmp_path / name
    run.mkdir()
    monkeypatch.chdir(run)
    trainers = []
    orig = T.Trainer.train

    def keep(self):
        trainers.append(self)
        return orig(self)
    monkeypatch.setattr(T.Trainer, "train", keep)
    torch.manual_seed(1)
    train.main(["--train_dir", str(tmp_path / "train"), "--valid_dir", str(tmp_path / "train"), "-W", "128", "-H", "128", "-s", "stem",
                "--labels", str(tmp_path / "labels.json"), "-b", "4", "-e", "2", "--decode_workers", "3"] + extra)
    out = capsys.readouterr().out
    return trainers[0], out


def test_train_with_the_cache_equals_train_without(golden_dir, tmp_path, monkeypatch, capsys):
    """Two fp32 epochs of `train` over a directory, same seeds, with --cache_images and without: bitwise identical weights and Adam state,
    the same validation line, and the prefill line printed."""
    from tests.helpers import write_evaluate16_dir
    g = np.load(golden_dir / "evaluate16.npz")
    write_evaluate16_dir(g, tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr_a, out_a = _train_run(tmp_path, "plain", [], monkeypatch, capsys)
    tr_b, out_b = _train_run(tmp_path, "cached", ["--cache_images", "0.5"], monkeypatch, capsys)
    assert tr_a.cache is None and tr_b.cache is not None
    assert re.search(r"image cache: 16 images, 0\.02 GB in [0-9.]+ s, 0 left on the host path", out_b), out_b
    st = tr_b.cache.stats()
    assert st["misses"] == 0 and st["hits"] == 2 * 16 + 16                          # two epochs of 4 x 4 + one validation pass
    val_a = [ln for ln in out_a.splitlines() if ln.startswith("validation")]
    val_b = [ln for ln in out_b.splitlines() if ln.startswith("validation")]
    assert val_a and val_a == val_b
    assert [ln for ln in out_a.splitlines() if ln.startswith("epoch")] == [ln for ln in out_b.splitlines() if ln.startswith("epoch")]
    assert torch.equal(tr_a.net.flat_params, tr_b.net.flat_params)
    assert torch.equal(tr_a.step.exp_avg, tr_b.step.exp_avg) and torch.equal(tr_a.step.exp_avg_sq, tr_b.step.exp_avg_sq)
