"""Crop training at the tile scale on the GPU (sd_preprocess_images_window / _list_window: k_window_h, k_window_h_list, k_window_v_norm,
k_window_v_u8) against Pillow itself -- Image.resize(canvas, BILINEAR).crop(window) -> to_tensor -> Normalize, bit for bit --, against the
library's own full-canvas resize, against the tiles inference cuts, against the existing entry points (grid 1x1; the later stages fed the
Pillow window), the origin clamps, TrainAugmentation with `--train_tiles` end to end and a few steps of `train`."""
import functools
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.affine_ref import PARAMS
from tests.window_ref import B, CASES, FREE_CASES, canvas_of, normalize, origins5, pil_window, sources

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLIPS = [0, 1, 2, 3, 1]
ALL_CASES = [(src, size, canvas_of(size, grid, overlap)) for src, size, grid, overlap in CASES] + FREE_CASES


@functools.lru_cache(maxsize=None)
def _case(src, size, canvas):
    """Images, origins and the Pillow windows of one (source shape, window size, canvas): computed once, read only."""
    imgs = sources(src)
    origins = origins5(canvas, size)
    windows = np.stack([pil_window(imgs[b], canvas, origins[b], size) for b in range(B)])
    for a in (imgs, windows):
        a.setflags(write=False)
    return imgs, origins, windows


def _arena(imgs, seed=1):
    from tests.test_gpu_image_cache import _arena_with
    arena, addrs = _arena_with(list(imgs), np.random.default_rng(seed))
    assert all(a % 2 == 1 for a in addrs)                                       # odd byte offsets inside one arena tensor
    return arena, torch.tensor(addrs, dtype=torch.int64, device=DEV)


def _jitter(n, seed=4):
    from structuredetector_amd.data.augment import jitter_words
    rng = np.random.default_rng(seed)
    jit = [jitter_words(list(rng.permutation(4)), *rng.uniform(0.75, 1.25, 2), rng.uniform(0.85, 1.15), rng.uniform(-0.05, 0.05)) for _ in range(n)]
    return [w for w, _ in jit], [f for _, f in jit]


def _warps(size, n):
    from structuredetector_amd.data.augment import affine_inverse_matrix
    return [affine_inverse_matrix(size, a, s, (tx, ty)) for a, s, tx, ty in PARAMS[1:1 + n]]


def _mosaic(size, n):
    """Every image a mosaic of itself and three others of the batch, around a centre off the block and thread grid."""
    from structuredetector_amd.data.augment import mosaic_tiles
    W, H = size
    rows = [mosaic_tiles(size, b, (W // 2 + 3 - b, H // 2 + 1 + b, ((b + 1) % n, (b + 2) % n, b))) for b in range(n)]
    return [r[0] for r in rows], [r[1] for r in rows]


def _stage_sets(size, n):
    """(name, keyword arguments) of flips, jitter, warp and mosaic alone, and of all of them together."""
    flips, jitter, warps, mosaic = FLIPS[:n], _jitter(n), _warps(size, n), _mosaic(size, n)
    return [("flips", dict(flips=flips)), ("jitter", dict(jitter=jitter)), ("affine", dict(affine=warps)), ("mosaic", dict(mosaic=mosaic)),
            ("all", dict(flips=flips, jitter=jitter, affine=warps, mosaic=mosaic))]


@pytest.mark.parametrize("src,size,canvas", ALL_CASES)
def test_window_matches_pillow_bitwise_packed_and_list(src, size, canvas):
    """Normalize of Pillow's cropped resize is the reference; nothing under test computes it."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    imgs, origins, windows = _case(src, size, canvas)
    assert len(set(origins)) == B or canvas == size                             # a different origin per image
    packed = preprocess_images(torch.tensor(imgs, device=DEV), size, window=(canvas, origins)).cpu()
    arena, table = _arena(imgs)
    listed = preprocess_image_list(table, src[0], src[1], size, window=(canvas, origins)).cpu()
    del arena
    assert packed.shape == listed.shape == (B, 3, size[1], size[0])
    for b in range(B):
        want = normalize(windows[b])
        assert torch.equal(packed[b], want), f"packed: image {b} origin {origins[b]}: {(packed[b] != want).sum().item()} values differ"
        assert torch.equal(listed[b], want), f"list: image {b} origin {origins[b]}: {(listed[b] != want).sum().item()} values differ"


@pytest.mark.parametrize("src,size,canvas", ALL_CASES)
def test_window_equals_the_slice_of_the_librarys_full_canvas(src, size, canvas):
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    imgs, origins, _ = _case(src, size, canvas)
    x = torch.tensor(imgs, device=DEV)
    full = preprocess_images(x, canvas)
    (w, h) = size
    want = torch.stack([full[b, :, y0:y0 + h, x0:x0 + w] for b, (x0, y0) in enumerate(origins)])
    assert torch.equal(preprocess_images(x, size, window=(canvas, origins)), want)
    arena, table = _arena(imgs, seed=2)
    assert torch.equal(preprocess_image_list(table, src[0], src[1], size, window=(canvas, origins)), want)
    del arena


# (inference refuses an overlap above half the smaller tile side, so the 64 x 48 tiles of CASES[3] cannot be cut with overlap 32: the
# anisotropic canvas here is 3x2 tiles of 64 x 64, 128 x 96)
@pytest.mark.parametrize("src,size,grid,overlap", CASES[:3] + [((61, 333), (64, 64), (3, 2), 32)])
def test_windows_at_the_tile_origins_are_the_tiles_inference_sees(src, size, grid, overlap):
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    from structuredetector_amd.model.tiles import tile_views
    from structuredetector_amd.utils.args import tile_canvas, tile_origins
    (w, h) = size
    canvas = tile_canvas(w, h, grid, overlap)
    imgs = sources(src)
    x = torch.tensor(imgs, device=DEV)
    tiles = tile_views(preprocess_images(x, canvas), grid, overlap)
    arena, table = _arena(imgs, seed=3)
    for t, (row, col) in enumerate(tile_origins(w, h, grid, overlap)):
        origins = [(col, row)] * B
        assert torch.equal(preprocess_images(x, size, window=(canvas, origins)), tiles[t * B:(t + 1) * B]), (t, row, col)
        assert torch.equal(preprocess_image_list(table, src[0], src[1], size, window=(canvas, origins)), tiles[t * B:(t + 1) * B]), (t, row, col)
    del arena


def test_a_wide_source_takes_fewer_than_four_rows_per_block():
    """8 x 6000 source, 64-wide window, grid 1x1: the column span is the whole 6000-pixel row, 18000 bytes, so a block of the list kernel
    stages three rows (8 rows: blocks of 3, 3 and 2)."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images, window_extents
    assert window_extents(6000, 64, 64) == 6000 and (65536 - 32) // (6000 * 3) == 3
    imgs = sources((8, 6000), n=2)
    x = torch.tensor(imgs, device=DEV)
    want = preprocess_images(x, (64, 64))
    for b in range(2):
        assert torch.equal(want[b].cpu(), normalize(pil_window(imgs[b], (64, 64), (0, 0), (64, 64))))
    origins = [(0, 0)] * 2
    assert torch.equal(preprocess_images(x, (64, 64), window=((64, 64), origins)), want)
    arena, table = _arena(imgs, seed=5)
    assert torch.equal(preprocess_image_list(table, 8, 6000, (64, 64), window=((64, 64), origins)), want)
    del arena


@pytest.mark.parametrize("src,size", [((150, 201), (64, 64)), ((61, 333), (70, 33))])
def test_grid_1x1_at_the_origin_is_the_existing_entry_point(src, size):
    """(70, 33): a width that is no multiple of 4 (the byte-store branch of the warp and mosaic kernels)."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    imgs = sources(src)
    x = torch.tensor(imgs, device=DEV)
    arena, table = _arena(imgs, seed=6)
    window = (size, [(0, 0)] * B)
    for name, kw in [("plain", {})] + _stage_sets(size, B):
        want = preprocess_images(x, size, **kw)
        assert torch.equal(preprocess_images(x, size, window=window, **kw), want), name
        assert torch.equal(preprocess_image_list(table, src[0], src[1], size, window=window, **kw), want), name
    del arena


@pytest.mark.parametrize("src,size,canvas", [ALL_CASES[0], ALL_CASES[3]])
def test_stages_on_a_window_equal_the_existing_entry_points_on_the_pillow_window(src, size, canvas):
    """The later stages see the window as they see a resized image: the existing entry points fed the Pillow window bytes as (B, h, w, 3)
    sources at out_size = (w, h) -- an identity resize -- give the same tensor."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    imgs, origins, windows = _case(src, size, canvas)
    x, wx = torch.tensor(imgs, device=DEV), torch.tensor(windows, device=DEV)
    assert torch.equal(preprocess_images(wx, size).cpu(), torch.stack([normalize(u) for u in windows]))     # the identity, checked
    arena, table = _arena(imgs, seed=7)
    for name, kw in _stage_sets(size, B):
        want = preprocess_images(wx, size, **kw)
        assert torch.equal(preprocess_images(x, size, window=(canvas, origins), **kw), want), name
        assert torch.equal(preprocess_image_list(table, src[0], src[1], size, window=(canvas, origins), **kw), want), name
    del arena


def test_origins_out_of_range_are_clamped():
    """The device table cannot be checked on the host: an origin one past the end of its range (and far outside it) gives exactly the
    clamped origin's output."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    src, size, canvas = ALL_CASES[0]
    imgs, _, _ = _case(src, size, canvas)
    mx, my = canvas[0] - size[0], canvas[1] - size[1]
    wild = [(mx + 1, my + 1), (-1, -1), (mx + 1, 3), (2**31 - 1, -2**31), (5, my + 1000)]
    tame = [(min(max(x0, 0), mx), min(max(y0, 0), my)) for x0, y0 in wild]
    assert tame == [(mx, my), (0, 0), (mx, 3), (mx, 0), (5, my)]
    x = torch.tensor(imgs, device=DEV)
    arena, table = _arena(imgs, seed=8)
    jitter = _jitter(B)
    for kw in ({}, dict(flips=FLIPS, jitter=jitter)):
        want = preprocess_images(x, size, window=(canvas, tame), **kw)
        got = preprocess_images(x, size, window=(canvas, wild), **kw)
        got_list = preprocess_image_list(table, src[0], src[1], size, window=(canvas, wild), **kw)
        torch.cuda.synchronize()                                                # the calls and the launches succeeded
        assert torch.equal(got, want) and torch.equal(got_list, want)
    del arena


# ---- TrainAugmentation end to end -----------------------------------------------------------------------------------------------
def _ann_rows(ann):
    return [(o.name, o.x, o.y, [(p.kind, p.x, p.y) for p in o.parts]) for o in ann.objects]


def _hand_composition(aug, raw, n, groups):
    """What `aug(batch, annotations)` must give for the raw (image tensor, annotation) items, by replaying its draws (the caller seeded the
    generator) and composing by hand: Pillow windows, the existing entry points on them (an identity resize), and the host annotation
    rules in the chain's order."""
    from structuredetector_amd.data import preprocess_images
    from structuredetector_amd.data.augment import _Objects, affine_forward_matrix, affine_inverse_matrix, mosaic_tiles
    from structuredetector_amd.utils.args import tile_canvas
    from structuredetector_amd.utils.misc import affine_annotation, clip_annotation, hflip_annotation, mosaic_annotation, vflip_annotation
    W, H = aug.size
    flips, jitter = aug.draws_for(n)
    warps = aug.affine_draws_for(n)
    mosaics = aug.mosaic_draws_for(n, groups)
    u = torch.rand(n, 2, dtype=torch.float64).tolist()                          # the window draw, written out
    Wc, Hc = tile_canvas(W, H, aug.train_tiles, aug.tile_overlap)
    origins = [(int(ux * (Wc - W + 1)), int(uy * (Hc - H + 1))) for ux, uy in u]
    assert all(0 <= x0 <= Wc - W and 0 <= y0 <= Hc - H for x0, y0 in origins)
    out = torch.empty((n, 3, H, W))
    anns = [a.clone() for _, a in raw]
    for idx in groups:
        windows = np.stack([pil_window(raw[i][0].numpy(), (Wc, Hc), origins[i], (W, H)) for i in idx])
        kw = {}
        if flips is not None:
            kw["flips"] = [flips[i] for i in idx]
            kw["jitter"] = ([jitter[0][i] for i in idx], [jitter[1][i] for i in idx])
        if warps is not None:
            kw["affine"] = [affine_inverse_matrix((W, H), a, s, (tx, ty)) for a, s, tx, ty in (warps[i] for i in idx)]
        if mosaics is not None:
            where = {i: k for k, i in enumerate(idx)}
            tiles = {i: mosaic_tiles((W, H), i, mosaics[i]) for i in idx}
            kw["mosaic"] = ([[*tiles[i][0][:2], *(where[s] for s in tiles[i][0][2:])] for i in idx], [tiles[i][1] for i in idx])
        out[idx] = preprocess_images(torch.tensor(windows, device=DEV), (W, H), **kw).cpu()
        for i in idx:
            hin, win = raw[i][0].shape[:2]
            anns[i].img_size = anns[i].img_size or (win, hin)
            anns[i].resize((win, hin), (Wc, Hc))
            affine_annotation(anns[i], [1, 0, -origins[i][0], 0, 1, -origins[i][1]], (W, H))
        if mosaics is not None:
            resized = {i: _Objects(anns[i].objects) for i in idx}
            for i in idx:
                if mosaics[i] is not None:
                    geom, _, forward, rects = tiles[i]
                    mosaic_annotation(anns[i], [resized[s] for s in geom[2:]], forward, rects)
        for i in idx:
            if warps is not None:
                a, s, tx, ty = warps[i]
                affine_annotation(anns[i], affine_forward_matrix((W, H), a, s, (tx, ty)), (W, H))
            if flips is not None and flips[i] & 1:
                hflip_annotation(anns[i], (W, H))
            if flips is not None and flips[i] & 2:
                vflip_annotation(anns[i], (W, H))
            clip_annotation(anns[i], (W, H))
    return out, anns, origins


@pytest.mark.parametrize("extra", [dict(no_augmentation=True), dict(no_augmentation=False),
                                   dict(no_augmentation=False, aug_rotate=15.0, aug_scale=0.1, aug_mosaic=0.6)], ids=["window", "jitter_flips", "all"])
def test_train_augmentation_with_train_tiles_on_a_mixed_size_batch(golden_dir, tmp_path, extra):
    from structuredetector_amd.data import BatchFeeder, CropDataset, DeviceImageCache, ImageList, TrainAugmentation
    from tests.helpers import EVAL16_LABELS, EVAL16_PARTS, write_evaluate16_dir
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    args = Namespace(labels=EVAL16_LABELS, parts=EVAL16_PARTS, width=128, height=96, anchor_name="stem", train_tiles="2x2", tile_overlap=32,
                     device=torch.device(DEV, torch.cuda.current_device()), **extra)
    ds = CropDataset(args, tmp_path / "train", raw=True)
    picks = [0, 1, 2, 3, 5, 8, 13, 4]
    raw = [ds[j] for j in picks]
    n = len(raw)
    aug = TrainAugmentation(args)
    assert aug.train_tiles == (2, 2)
    batch = next(iter(BatchFeeder(ds, [picks], DEV, workers=2)))
    groups = [idx for idx, _ in batch.groups.values()]
    assert len(groups) > 1                                                      # several source sizes in the batch
    torch.manual_seed(31)
    want, want_anns, origins = _hand_composition(aug, raw, n, groups)
    state = torch.get_rng_state()
    torch.manual_seed(31)
    got, anns = aug(batch, batch.annotations)
    assert torch.equal(torch.get_rng_state(), state)                            # the same draws, no more
    assert got.shape == (n, 3, 96, 128) and torch.equal(got.cpu(), want)
    assert [_ann_rows(a) for a in anns] == [_ann_rows(a) for a in want_anns]
    if extra["no_augmentation"]:                                                # the window rule written out: scale to the canvas, shift, drop
        dropped = 0
        for i, (img, ann) in enumerate(raw):
            (hin, win), (x0, y0) = img.shape[:2], origins[i]
            expect = []
            for o in ann.objects:
                pts = [((p.x * (224 / win) + 0.5) - x0, (p.y * (160 / hin) + 0.5) - y0) for p in (o.anchor, *o.parts)]
                inside = [0 <= x < 128 and 0 <= y < 96 for x, y in pts]
                dropped += len(pts) - (sum(inside) if inside[0] else 0)
                if inside[0]:
                    expect.append([pts[0]] + [p for p, k in zip(pts[1:], inside[1:]) if k])
            have = [[(o.x + 0.5, o.y + 0.5)] + [(p.x + 0.5, p.y + 0.5) for p in o.parts] for o in anns[i].objects]
            assert len(have) == len(expect) and all(len(h) == len(e) for h, e in zip(have, expect)), i
            for h, e in zip(have, expect):
                for (hx, hy), (ex, ey) in zip(h, e):
                    assert abs(min(max(ex - 0.5, 0), 127) - (hx - 0.5)) <= 1e-9 and abs(min(max(ey - 0.5, 0), 95) - (hy - 0.5)) <= 1e-9
        assert dropped > 0                                                      # a window shows part of the frame: something left it
    # the same batch through the device image cache: pointer tables instead of packed stacks, bit-identical
    cache = DeviceImageCache(1 << 28, DEV)
    cache.prefill(ds, workers=2)
    cached = next(iter(BatchFeeder(ds, [picks], DEV, workers=2, cache=cache)))
    assert all(isinstance(v, ImageList) for _, v in cached.groups.values())
    torch.manual_seed(31)
    got_cached, anns_cached = aug(cached, cached.annotations)
    assert torch.equal(got_cached, got) and [_ann_rows(a) for a in anns_cached] == [_ann_rows(a) for a in anns]


def test_validation_augmentation_never_draws_a_window():
    from structuredetector_amd.data import ValidationAugmentation
    args = Namespace(width=128, height=96, train_tiles="2x2", tile_overlap=32, device=torch.device(DEV))
    state = torch.get_rng_state()
    assert ValidationAugmentation(args).window_draws_for(4) is None and torch.equal(torch.get_rng_state(), state)


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
    train.main(["--train_dir", str(tmp_path / "train"), "-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "-b", "4",
                "-e", "1", "--steps", "2", "--decode_workers", "2", "--train_tiles", "2x2", "--tile_overlap", "32"] + extra)
    monkeypatch.setattr(T.Trainer, "train", orig)
    return trainers[0], capsys.readouterr().out


def test_train_cli_with_train_tiles_over_a_png_json_directory(golden_dir, tmp_path, monkeypatch, capsys):
    """Two steps of `train --train_tiles 2x2` at 128 x 128 (the size the other CLI tests train at; the overlap must hold for 96 x 96, the
    smallest multi-scale size) with and without --cache_images: finite losses, identical between the two runs."""
    import re

    from tests.helpers import write_evaluate16_dir
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr_a, out_a = _train_run(tmp_path, "plain", [], monkeypatch, capsys)
    tr_b, out_b = _train_run(tmp_path, "cached", ["--cache_images", "0.5"], monkeypatch, capsys)
    assert tr_a.cache is None and tr_b.cache is not None and tr_a.augment.train_tiles == (2, 2)
    assert "train tiles:" in out_a and "evaluate --tiles" in out_a
    lines_a = [ln for ln in out_a.splitlines() if ln.startswith("epoch 0:")]
    lines_b = [ln for ln in out_b.splitlines() if ln.startswith("epoch 0:")]
    assert len(lines_a) == 1 and lines_a == lines_b and "(2 steps)" in lines_a[0], (out_a, out_b)
    losses = [float(v) for v in re.findall(r"(?:total|hm|offset|embedding) (\S+)", lines_a[0])]
    assert len(losses) == 4 and np.isfinite(losses).all() and losses[0] > 0, lines_a
    assert torch.isfinite(tr_a.net.flat_params).all() and torch.equal(tr_a.net.flat_params, tr_b.net.flat_params)
