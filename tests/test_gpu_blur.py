"""Gaussian blur on the GPU (sd_blur_u8: k_blur_h, k_blur_v; sd_preprocess_images_blur / _list_blur; k_u8_norm) against
tests/blur_ref.py -- the numpy restatement that tests/test_blur_cpu.py pins to Pillow byte for byte -- bit for bit: the stand-alone stage
over sizes around the 80-pixel / 64-row / 256-byte tiles and the 3 (R + 1) halo, the chain forms against the hand composition of the
existing entry points and blur_ref, a null table against the existing entry points, `TrainAugmentation` with `--aug_blur` against
Pillow's own chain, and `train --aug_blur`."""
import functools
import json
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.blur_ref import blur_params, blur_ref, box_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN = torch.tensor((0.485, 0.456, 0.406))[:, None, None]
STD = torch.tensor((0.229, 0.224, 0.225))[:, None, None]

# (height, width): a line shorter than R + 1, H = 1 and W = 1, sizes that are no multiple of a tile and cross its boundary, several strips;
# both orientations; 64 x 96 and 150 x 176 have 3 W a multiple of 16 (the 16-byte path), the latter over 3 x 3 tiles with halos on both sides
SIZES = [(1, 1), (2, 3), (5, 7), (3, 40), (33, 17), (64, 96), (130, 70)]
SHAPES = SIZES + [(w, h) for h, w in SIZES if h != w] + [(150, 176)]
MIX = [0.0, 0.3, 1.0, 2.5, 8.0]                                     # copy, R = 0 with the edge weight only, R = 0, R = 2, R = SD_BLUR_MAX_RADIUS


@functools.lru_cache(maxsize=None)
def _stage_case(shape):
    """Images, table rows and the expected bytes of one shape: computed once, read only."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in MIX]
    rows = [box_params(r) for r in MIX]
    want = [blur_ref(a, r) for a, r in zip(imgs, MIX)]
    for fill, r in ((0, 2.5), (255, 8.0)):                          # constant images stay constant
        imgs.append(np.full((h, w, 3), fill, np.uint8)); rows.append(box_params(r)); want.append(imgs[-1].copy())
        assert np.array_equal(blur_ref(imgs[-1], r), imgs[-1])
    for bad_r, r in ((100, 8.0), (-3, 0.3), (2 ** 31 - 1, 8.0)):    # R out of range: the output of the clamped row (weights legal at that R)
        _, ww, fw = box_params(r)
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        imgs.append(a); rows.append((bad_r, ww, fw)); want.append(blur_params(a, min(max(bad_r, 0), 7), ww, fw))
    imgs, want = np.stack(imgs), np.stack(want)
    imgs.setflags(write=False); want.setflags(write=False)
    return imgs, rows, want


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_sd_blur_u8_matches_the_reference_bitwise(shape):
    from structuredetector_amd.data import blur_images
    imgs, rows, want = _stage_case(shape)
    x = torch.tensor(imgs, device=DEV)
    got = blur_images(x, rows).cpu().numpy()
    assert np.array_equal(x.cpu().numpy(), imgs)                     # the input is read only
    for b in range(len(rows)):
        bad = got[b] != want[b]
        assert not bad.any(), f"{shape} row {b} {rows[b]}: {bad.sum()} bytes differ, first at {np.argwhere(bad)[0].tolist()}"
    # the same rows in another order: a block reads its own image's row of the table
    perm = list(range(len(rows)))[::-1]
    again = blur_images(torch.tensor(imgs[perm], device=DEV), [rows[i] for i in perm]).cpu().numpy()
    assert np.array_equal(again, want[perm])


def test_sd_blur_u8_on_views_that_are_not_16_byte_aligned():
    """A width whose rows are whole 16-byte chunks, at a base address that is not: the byte path gives the same bytes."""
    from structuredetector_amd import _lib as L
    imgs, rows, want = _stage_case((64, 96))
    B, H, W = imgs.shape[:3]
    n = imgs.size
    arena_in = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
    arena_out = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
    arena_in[5:5 + n].copy_(torch.tensor(imgs, device=DEV).reshape(-1))
    table = torch.tensor(np.asarray(rows, dtype=np.int64).astype(np.int32), device=DEV)
    lib = L.lib()
    ws = L.workspace(lib.sd_blur_workspace_bytes(B, H, W), torch.device(DEV, torch.cuda.current_device()))
    L.check(lib.sd_blur_u8(arena_in.data_ptr() + 5, arena_out.data_ptr() + 3, B, H, W, table.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()),
            "sd_blur_u8")
    out = arena_out.cpu().numpy()
    assert np.array_equal(out[3:3 + n].reshape(imgs.shape), want)
    assert not out[:3].any() and not out[3 + n:].any()               # nothing outside the images is written


# ---- the chain forms -------------------------------------------------------------------------------------------------------------
SRC, OUT, NB = (40, 56), (32, 32), 4                                 # sources (height, width), network input (width, height), batch
RADII = [0.0, 0.7, 2.0, 5.0]                                         # one sharp image in the batch


@functools.lru_cache(maxsize=None)
def _sources():
    imgs = np.random.default_rng(77).integers(0, 256, (NB, *SRC, 3), dtype=np.uint8)
    imgs.setflags(write=False)
    return imgs


def _geometry(name):
    from structuredetector_amd.data import letterbox_geometry
    if name == "window":
        return dict(window=((48, 40), [(0, 0), (16, 8), (7, 3), (11, 5)]))
    if name == "letterbox":
        box = letterbox_geometry((SRC[1], SRC[0]), OUT)
        assert box[0] < OUT[0] or box[1] < OUT[1]                    # there are bars
        return dict(letterbox=box)
    return {}


def _stage_sets():
    """(name, the stages in front of the blur, the stages behind it)."""
    from tests.test_gpu_train_tiles import FLIPS, _jitter, _mosaic, _warps
    flips, jitter, warps, mosaic = FLIPS[:NB], _jitter(NB), _warps(OUT, NB), _mosaic(OUT, NB)
    assert any(f & 1 for f in flips) and any(f & 2 for f in flips)
    return [("plain", {}, {}), ("flips", {}, dict(flips=flips)), ("jitter", {}, dict(jitter=jitter)),
            ("jitter_flips", {}, dict(flips=flips, jitter=jitter)), ("affine", dict(affine=warps), {}), ("mosaic", dict(mosaic=mosaic), {}),
            ("affine_jitter_flips", dict(affine=warps), dict(flips=flips, jitter=jitter)),
            ("all", dict(affine=warps, mosaic=mosaic), dict(flips=flips, jitter=jitter))]


def _bytes(t):
    """(B, 3, H, W) normalised fp32 -> (B, H, W, 3) uint8: un-normalising is exact to well under half a byte step."""
    return (t.cpu() * STD + MEAN).mul(255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()


def _table():
    from tests.test_gpu_image_cache import _arena_with
    arena, addrs = _arena_with(list(_sources()), np.random.default_rng(5))
    return arena, torch.tensor(addrs, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_chain_forms_equal_the_hand_composition(geometry):
    """The existing 8-bit chain up to the warp (its bytes read back from the existing entry point), blur_ref on the host, then the
    existing jitter / flips / normalise on those bytes (an identity resize): the packed and the list form give that tensor bit for bit."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    x = torch.tensor(_sources(), device=DEV)
    arena, table = _table()
    geom = _geometry(geometry)
    rows = [box_params(r) for r in RADII]
    for name, front, behind in _stage_sets():
        head = preprocess_images(x, OUT, **geom, **front)
        u8 = _bytes(head)
        assert torch.equal(preprocess_images(torch.tensor(u8, device=DEV), OUT), head), name                 # the bytes, and the identity resize
        blurred = np.stack([blur_ref(u8[b], RADII[b]) for b in range(NB)])
        assert np.array_equal(blurred[0], u8[0]) and (blurred[1:] != u8[1:]).any()
        want = preprocess_images(torch.tensor(blurred, device=DEV), OUT, **behind)
        got = preprocess_images(x, OUT, **geom, **front, **behind, blur=rows)
        assert torch.equal(got, want), f"packed {geometry} {name}: {(got != want).sum().item()} values differ"
        got = preprocess_image_list(table, SRC[0], SRC[1], OUT, **geom, **front, **behind, blur=rows)
        assert torch.equal(got, want), f"list {geometry} {name}: {(got != want).sum().item()} values differ"
    del arena


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_a_null_table_is_the_existing_entry_point_bit_for_bit(geometry):
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    from structuredetector_amd.data.augment import _MEAN, _STD
    from tests.helpers import call_legacy_preprocess_form as _preprocess_blur
    x = torch.tensor(_sources(), device=DEV)
    arena, table = _table()
    geom = _geometry(geometry)
    for name, front, behind in _stage_sets():
        kw = dict(flips=None, jitter=None, affine=None, mosaic=None, window=None, letterbox=None)
        kw.update(geom); kw.update(front); kw.update(behind)
        args = (NB, SRC[0], SRC[1], OUT, kw["flips"], _MEAN, _STD, kw["jitter"], kw["affine"], kw["mosaic"], kw["window"], kw["letterbox"], None, x.device)
        want = preprocess_images(x, OUT, **geom, **front, **behind)
        assert torch.equal(_preprocess_blur("sd_preprocess_images_blur", x.data_ptr(), *args), want), name
        want = preprocess_image_list(table, SRC[0], SRC[1], OUT, **geom, **front, **behind)
        assert torch.equal(_preprocess_blur("sd_preprocess_images_list_blur", table.data_ptr(), *args), want), name
    del arena


def test_chain_rejects_what_its_geometry_rejects():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import preprocess_images
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    one = [box_params(1.0)]
    with pytest.raises(L.SdError, match="do not combine"):
        preprocess_images(x, (8, 8), letterbox=(8, 8, 0, 0), window=((8, 8), [(0, 0)]), blur=one)
    with pytest.raises(L.SdError, match="does not lie inside"):
        preprocess_images(x, (8, 8), letterbox=(8, 8, 1, 0), blur=one)
    with pytest.raises(L.SdError, match="one row"):
        preprocess_images(x, (8, 8), blur=one * 2)


# ---- the augmentation class and the CLI ------------------------------------------------------------------------------------------
def _pillow_chain(img, size, r, jit, hflip, vflip):
    """Resize -> GaussianBlur -> ColorJitter -> flips -> to_tensor -> Normalize, every image operation Pillow's own."""
    from PIL import Image, ImageFilter
    from tests.test_gpu_pipeline import pil_color_jitter
    im = Image.fromarray(img).resize(size, Image.BILINEAR)
    if r > 0:
        im = im.filter(ImageFilter.GaussianBlur(r))
    im = pil_color_jitter(im, *jit)
    if hflip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if vflip:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    return torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).to(torch.float32).div(255).sub(MEAN).div(STD)


def test_train_augmentation_with_aug_blur_equals_the_pillow_chain():
    from structuredetector_amd.data import TrainAugmentation
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    size = (96, 64)
    rng = np.random.default_rng(9)
    imgs = [rng.integers(0, 256, (60, 80, 3), dtype=np.uint8) for _ in range(4)]
    make_anns = lambda: [ImageAnnotation(f"{i}.png", [Object("bean", Keypoint("stem", 10.0 * i + 1, 5.0 * i + 2), [])]) for i in range(4)]
    common = dict(width=size[0], height=size[1], no_augmentation=False, device=torch.device(DEV))
    outs = {}
    for blur in (2.0, 0.0):
        aug = TrainAugmentation(Namespace(**common, aug_blur=blur))
        torch.manual_seed(21)
        flips, (words, factors) = aug.draws_for(4)                   # the draws the call below makes, in its order
        radii = aug.blur_draws_for(4)
        torch.manual_seed(21)
        out, anns = aug(imgs, make_anns())
        if blur:
            assert any(r > 0 for r in radii) and any(r == 0 for r in radii) and all(r <= 2.0 for r in radii)
        else:
            assert radii is None
        for i in range(4):
            order = [(words[i] >> (2 * k)) & 3 for k in range(4)]
            jit = (order, *factors[i], ((words[i] >> 8) & 255,))
            want = _pillow_chain(imgs[i], size, radii[i] if radii else 0.0, jit, bool(flips[i] & 1), bool(flips[i] & 2))
            assert torch.equal(out[i].cpu(), want), f"aug_blur {blur} image {i}: {(out[i].cpu() != want).sum().item()} values differ"
        outs[blur] = (out.cpu(), [(a.objects[0].x, a.objects[0].y) for a in anns])
    assert outs[2.0][1] == outs[0.0][1]                              # photometric: the annotations are those of the sharp chain
    assert not torch.equal(outs[2.0][0], outs[0.0][0])


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
    train.main(["--train_dir", str(tmp_path / "train"), "-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "-b", "4",
                "-e", "1", "--steps", "2", "--decode_workers", "2", "--aug_blur", "2"] + extra)
    monkeypatch.setattr(T.Trainer, "train", orig)
    return trainers[0], capsys.readouterr().out


def _epoch_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("epoch 0:")]
    assert len(lines) == 1 and "(2 steps)" in lines[0], out
    losses = [float(v) for v in re.findall(r"(?:total|hm|offset|embedding) (\S+)", lines[0])]
    assert len(losses) == 4 and np.isfinite(losses).all() and losses[0] > 0, lines
    return lines[0]


def test_train_cli_with_aug_blur_with_and_without_the_image_cache(golden_dir, tmp_path, monkeypatch, capsys):
    """Two steps of `train --aug_blur 2` from a PNG + JSON directory: finite losses, identical with and without --cache_images (the packed
    and the pointer-list form of the chain)."""
    from tests.helpers import write_evaluate16_dir
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr_a, out_a = _train_run(tmp_path, "plain", [], monkeypatch, capsys)
    tr_b, out_b = _train_run(tmp_path, "cached", ["--cache_images", "0.5"], monkeypatch, capsys)
    assert tr_a.cache is None and tr_b.cache is not None and tr_a.augment.blur == 2.0
    assert _epoch_line(out_a) == _epoch_line(out_b)
    assert torch.isfinite(tr_a.net.flat_params).all() and torch.equal(tr_a.net.flat_params, tr_b.net.flat_params)


@pytest.mark.parametrize("extra", [["--keep_aspect"], ["--train_tiles", "2x2", "--tile_overlap", "32"]], ids=["keep_aspect", "train_tiles"])
def test_train_cli_with_aug_blur_behind_the_other_geometries(golden_dir, tmp_path, monkeypatch, capsys, extra):
    from tests.helpers import write_evaluate16_dir
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr, out = _train_run(tmp_path, "run", extra, monkeypatch, capsys)
    _epoch_line(out)
    assert tr.augment.blur == 2.0 and torch.isfinite(tr.net.flat_params).all()
