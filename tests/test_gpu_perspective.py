"""Random perspective on the GPU (sd_perspective_u8: k_persp_u8; sd_preprocess_images_persp / _list_persp) against Pillow itself,
`Image.transform(size, PERSPECTIVE, coeffs, BILINEAR, fillcolor)`, bit for bit: the stand-alone stage over the store branches and the
border, wild rows through the clamps, the chain forms against the hand composition on PIL images behind the three geometries, a null
table against the blur forms, `TrainAugmentation` with `--aug_perspective` against Pillow's own chain with the annotations, and `train`."""
import ctypes as C
import functools
import json
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.affine_ref import FILL
from tests.mosaic_ref import FLIPS, batch_tables, pil_mosaic
from tests.perspective_ref import IDENTITY, affine_rows, hand_made, perspective_bilinear, pil_perspective, policy_coeffs
from tests.test_gpu_pipeline import MEAN, STD, pil_color_jitter

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 6

# (H, W): dword stores (W % 4 == 0) in one and several blocks; (33, 70) byte stores, a partial tile in both directions and the byte loads
# at the right border; (5, 7) where every tap is at a border
SHAPES = [(32, 64), (64, 96), (48, 128), (33, 70), (5, 7)]


def _mixed_rows(W, H):
    """B = 7: the identity, a pure-affine row, policy quads at D = 0.3 / 0.5 / 0.9, a denominator that changes sign, one that is exactly 0."""
    hand = hand_made(W, H)
    return [list(IDENTITY), affine_rows(W, H)[1], policy_coeffs(W, H, 0.3, 1)[0], policy_coeffs(W, H, 0.5, 2)[0], policy_coeffs(W, H, 0.9, 3)[0],
            list(hand["behind"]), list(hand["zero"])]


@functools.lru_cache(maxsize=None)
def _stage_case(shape):
    """Images, rows and Pillow's bytes of one shape: computed once, read only."""
    H, W = shape
    rows = _mixed_rows(W, H)
    imgs = np.random.default_rng(H * 1000 + W).integers(0, 256, (len(rows), H, W, 3), dtype=np.uint8)
    want = np.stack([pil_perspective(imgs[b], rows[b]) for b in range(len(rows))])
    imgs.setflags(write=False); want.setflags(write=False)
    return imgs, rows, want


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_sd_perspective_u8_matches_pillow_bitwise(shape):
    from structuredetector_amd.data import perspective_images
    imgs, rows, want = _stage_case(shape)
    x = torch.tensor(imgs, device=DEV)
    got = perspective_images(x, rows).cpu()
    assert torch.equal(x.cpu(), torch.from_numpy(imgs.copy()))                          # the input is read only
    for b in range(len(rows)):
        bad = (got[b].numpy() != want[b]).any(-1)
        assert torch.equal(got[b], torch.from_numpy(want[b].copy())), \
            f"{shape} row {b} {rows[b]}: {bad.sum()} pixels differ, first at {np.argwhere(bad)[0].tolist()}"
    assert torch.equal(got[0], x[0].cpu())                                              # the identity row is a copy
    # the same rows in another order: a block reads its own image's row of the table
    perm = list(range(len(rows)))[::-1]
    again = perspective_images(torch.tensor(imgs[perm], device=DEV), [rows[i] for i in perm]).cpu().numpy()
    assert np.array_equal(again, want[perm])


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_pure_affine_rows_equal_the_affine_path(shape):
    """a6 = a7 = 0: the bytes of k_affine_u8 with the same six coefficients (read back through the existing chain: an identity resize, the
    warp, Normalize) and Pillow's AFFINE transform."""
    from structuredetector_amd.data import perspective_images, preprocess_images
    H, W = shape
    rows = affine_rows(W, H)
    imgs = np.random.default_rng(W).integers(0, 256, (len(rows), H, W, 3), dtype=np.uint8)
    x = torch.tensor(imgs, device=DEV)
    got = perspective_images(x, rows)
    assert torch.equal(preprocess_images(got, (W, H)), preprocess_images(x, (W, H), affine=[r[:6] for r in rows]))
    from tests.affine_ref import pil_affine
    for b, r in enumerate(rows):
        assert np.array_equal(got[b].cpu().numpy(), pil_affine(imgs[b], r[:6])), (shape, b)


def test_wild_rows_stay_inside_their_image():
    """Nothing in a row is validated: huge, negative and non-finite-producing coefficients go through the inside test and the index clamps.
    The neighbouring images keep Pillow's bytes, a guard band around the output keeps its pattern, and the wild rows give what the
    definition says (an infinite or NaN position is fill)."""
    from structuredetector_amd import _lib as L
    H, W = 33, 70
    wild = [[1e300, -1e300, 1e308, -1e308, 1e300, 1e300, 1e300, -1e300], [-3.7, 2.2, 500.0, 1.9, -4.4, -300.0, 0.3, -0.2],
            [1e-300, 0.0, 35.0, 0.0, -1e-300, 16.0, -1e308, 1e308], [-1.0, 0.0, 69.999, 0.0, -1.0, 32.999, 0.0, 0.0]]
    tame = policy_coeffs(W, H, 0.5, 4)[0]
    rows = [tame, wild[0], tame, wild[1], wild[2], tame, wild[3], tame]
    n = len(rows)
    imgs = np.random.default_rng(5).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    size, guard = imgs.size, 4096
    arena = torch.full((size + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
    x = torch.tensor(imgs, device=DEV)
    table = torch.tensor(np.asarray(rows, dtype=np.float64), device=DEV)
    L.check(L.lib().sd_perspective_u8(x.data_ptr(), arena.data_ptr() + guard, n, H, W, table.data_ptr(), (C.c_ubyte * 3)(*FILL), L.stream()),
            "sd_perspective_u8")
    torch.cuda.synchronize()
    out = arena.cpu().numpy()
    assert (out[:guard] == 0xAB).all() and (out[guard + size:] == 0xAB).all()           # nothing outside the images is written
    assert np.array_equal(x.cpu().numpy(), imgs)
    got = out[guard:guard + size].reshape(imgs.shape)
    for b, row in enumerate(rows):
        want = pil_perspective(imgs[b], row) if row is tame else perspective_bilinear(imgs[b], row)[0]
        assert np.array_equal(got[b], want), f"row {b} {row}"
    assert (got[1] == np.asarray(FILL, np.uint8)).all()                                 # every position of the first wild row is outside


def test_in_place_and_bad_batches_are_refused():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import perspective_images
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=DEV)
    table = torch.tensor(np.asarray([IDENTITY] * 2), device=DEV)
    rc = L.lib().sd_perspective_u8(x.data_ptr(), x.data_ptr() + 3, 2, 8, 8, table.data_ptr(), (C.c_ubyte * 3)(*FILL), L.stream())
    assert rc == -1 and b"overlap" in L.lib().sd_last_error()
    with pytest.raises(L.SdError, match="one row of 8"):
        perspective_images(x, [IDENTITY])


# ---- the chain forms ---------------------------------------------------------------------------------------------------------------
CHAIN = [((33, 47), (96, 64)), ((33, 47), (70, 33)), ((160, 96), (96, 64)), ((160, 96), (70, 33))]     # source (H, W), network input (W, H)
RADII = [0.0, 0.7, 2.0, 5.0, 1.3, 8.0]                                                  # one sharp image in the batch


def _persp_rows(size):
    """One row per image of the batch: policy quads, a composed affine + perspective, a pure-affine row, a negative denominator, the identity."""
    from structuredetector_amd.data import affine_inverse_matrix, compose_affine_perspective
    W, H = size
    return [policy_coeffs(W, H, 0.3, 1)[0], compose_affine_perspective(affine_inverse_matrix(size, 17.3, 1.1, (3.25, -4.5)), policy_coeffs(W, H, 0.5, 2)[0]),
            affine_rows(W, H)[2], list(hand_made(W, H)["behind"]), policy_coeffs(W, H, 0.9, 3)[0], list(IDENTITY)]


def _geometry(name, src, size):
    """(keyword arguments of preprocess_images, the function that makes Pillow's frame of image b)."""
    from PIL import Image
    from tests.letterbox_ref import pil_frame
    from tests.window_ref import pil_window
    from structuredetector_amd.data import letterbox_geometry
    if name == "window":
        canvas = (size[0] + 24, size[1] + 16)
        origins = [(0, 0), (24, 16), (7, 3), (11, 5), (24, 0), (1, 15)]
        return dict(window=(canvas, origins)), lambda im, b: pil_window(im, canvas, origins[b], size)
    if name == "letterbox":
        box = letterbox_geometry((src[1], src[0]), size)
        assert box[0] < size[0] or box[1] < size[1]                                     # there are bars
        return dict(letterbox=box), lambda im, b: pil_frame(im, size)
    return {}, lambda im, b: np.asarray(Image.fromarray(im).resize(size, Image.BILINEAR)).copy()


def _finish(u8, flip, jit=None, radius=0.0):
    """[GaussianBlur] -> [ColorJitter] -> flips -> to_tensor -> Normalize of an (H, W, 3) uint8 image, on PIL images."""
    from PIL import Image, ImageFilter
    im = Image.fromarray(u8)
    if radius > 0:
        im = im.filter(ImageFilter.GaussianBlur(radius))
    if jit is not None:
        im = pil_color_jitter(im, *jit)
    if flip & 1:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if flip & 2:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    return torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).to(torch.float32).div(255).sub(MEAN).div(STD)


@pytest.mark.parametrize("src,size", CHAIN, ids=[f"{s[0]}x{s[1]}-{z[0]}x{z[1]}" for s, z in CHAIN])
@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_chain_forms_equal_the_hand_composition_on_pil_images(geometry, src, size):
    """resize | window | letterbox -> [mosaic] -> transform(PERSPECTIVE) -> [GaussianBlur] -> [ColorJitter] -> flips -> Normalize, every image
    operation Pillow's own; the packed and the list form give that tensor bit for bit."""
    from structuredetector_amd.data import blur_box_params, preprocess_image_list, preprocess_images
    from structuredetector_amd.data.augment import jitter_words
    from tests.test_gpu_image_cache import _arena_with
    rng = np.random.default_rng(src[0] * 131 + size[0])
    imgs = rng.integers(0, 256, (B, src[0], src[1], 3), dtype=np.uint8)
    kw, frame_of = _geometry(geometry, src, size)
    frames = [frame_of(imgs[b], b) for b in range(B)]
    geom, mats = batch_tables(size)
    composites = [pil_mosaic(frames, geom[b], mats[b]) for b in range(B)]
    rows = _persp_rows(size)
    jits = [([1, 0, 2, 3] if b % 2 else [0, 2, 3, 1], float(rng.uniform(0.75, 1.25)), float(rng.uniform(0.75, 1.25)), float(rng.uniform(0.85, 1.15)),
             float(rng.uniform(-0.05, 0.05))) for b in range(B)]
    words, factors = zip(*(jitter_words(*j) for j in jits))
    jitter, blur = (list(words), list(factors)), [blur_box_params(r) for r in RADII]
    x = torch.tensor(imgs, device=DEV)
    arena, addrs = _arena_with(list(imgs), np.random.default_rng(5))
    table = torch.tensor(addrs, dtype=torch.int64, device=DEV)
    for name, stages in (("none", {}), ("jitter", dict(jitter=jitter)), ("blur", dict(blur=blur)), ("mosaic", dict(mosaic=(geom, mats))),
                         ("mosaic_blur_jitter", dict(mosaic=(geom, mats), blur=blur, jitter=jitter))):
        base = composites if "mosaic" in stages else frames
        want = torch.stack([_finish(pil_perspective(base[b], rows[b]), FLIPS[b], jits[b] if "jitter" in stages else None,
                                    RADII[b] if "blur" in stages else 0.0) for b in range(B)])
        got = preprocess_images(x, size, FLIPS, persp=rows, **kw, **stages).cpu()
        assert torch.equal(got, want), f"packed {geometry} {name}: {(got != want).sum().item()} values differ"
        got = preprocess_image_list(table, src[0], src[1], size, FLIPS, persp=rows, **kw, **stages).cpu()
        assert torch.equal(got, want), f"list {geometry} {name}: {(got != want).sum().item()} values differ"
    got = preprocess_images(x, size, persp=rows, **kw).cpu()                           # flips = None
    assert torch.equal(got[1], _finish(pil_perspective(frames[1], rows[1]), 0))
    del arena


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_a_null_table_is_the_blur_form_bit_for_bit(geometry):
    from structuredetector_amd.data import blur_box_params, preprocess_images
    from structuredetector_amd.data.augment import _MEAN, _STD, affine_inverse_matrix
    from tests.helpers import call_legacy_preprocess_form as _preprocess_blur
    src, size = (33, 47), (70, 33)
    imgs = np.random.default_rng(3).integers(0, 256, (B, src[0], src[1], 3), dtype=np.uint8)
    x = torch.tensor(imgs, device=DEV)
    kw, _ = _geometry(geometry, src, size)
    warps = [affine_inverse_matrix(size, 10.0 * b, 1.0 + 0.05 * b, (b, -b)) for b in range(B)]
    for stages in ({}, dict(blur=[blur_box_params(r) for r in RADII]), dict(affine=warps), dict(affine=warps, blur=[blur_box_params(r) for r in RADII],
                                                                                               mosaic=batch_tables(size))):
        want = preprocess_images(x, size, FLIPS, **kw, **stages)
        got = _preprocess_blur("sd_preprocess_images_persp", x.data_ptr(), B, src[0], src[1], size, FLIPS, _MEAN, _STD, None, stages.get("affine"),
                               stages.get("mosaic"), kw.get("window"), kw.get("letterbox"), stages.get("blur"), x.device, None)
        assert torch.equal(got, want), (geometry, sorted(stages))


def test_persp_with_affine_is_refused():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    ident6 = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]]
    with pytest.raises(L.SdError, match="do not combine"):
        preprocess_images(x, (8, 8), persp=[IDENTITY], affine=ident6)
    with pytest.raises(L.SdError, match="do not combine"):
        preprocess_image_list(torch.tensor([x.data_ptr()], dtype=torch.int64, device=DEV), 8, 8, (8, 8), persp=[IDENTITY], affine=ident6)
    with pytest.raises(L.SdError, match="one row of 8"):
        preprocess_images(x, (8, 8), persp=[IDENTITY] * 2)
    # the library's own refusal, under the Python check
    lib = L.lib()
    ws = L.workspace(lib.sd_preprocess_blur_workspace_bytes(0, 1, 8, 8, 0, 8, 8, 0), x.device)
    t = torch.zeros(64, dtype=torch.float64, device=DEV)
    rc = lib.sd_preprocess_images_persp(x.data_ptr(), 0, 1, 8, 8, 0, 0, 8, 8, 0, 0, t.data_ptr(), t.data_ptr(), 3, t.data_ptr(), t.data_ptr(), 3, None,
                                        None, None, None, t.data_ptr(), t.data_ptr(), None, None, None, (C.c_ubyte * 3)(*FILL), (C.c_float * 3)(0, 0, 0),
                                        (C.c_float * 3)(1, 1, 1), t.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())
    assert rc == -1 and b"do not combine" in lib.sd_last_error()


# ---- the augmentation class and the CLI --------------------------------------------------------------------------------------------
def _rows(ann):
    return [(o.name, o.x, o.y, [(p.kind, p.x, p.y) for p in o.parts], o.box and (o.box.x_min, o.box.x_max, o.box.y_min, o.box.y_max)) for o in ann.objects]


def test_train_augmentation_with_aug_perspective_equals_the_pillow_chain_and_moves_the_annotations():
    from PIL import Image
    from structuredetector_amd.data import (TrainAugmentation, affine_forward_matrix, affine_inverse_matrix, compose_affine_perspective,
                                            perspective_coeffs)
    from structuredetector_amd.utils import (Box, ImageAnnotation, Keypoint, Object, affine_annotation, clip_annotation, hflip_annotation,
                                             perspective_annotation, vflip_annotation)
    W, H = size = (96, 64)
    rng = np.random.default_rng(9)
    shapes = [(60, 80), (45, 70), (60, 80), (45, 70), (60, 80), (60, 80)]               # two source sizes, interleaved
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    n = len(imgs)

    def make_anns():
        return [ImageAnnotation(f"{i}.png", [Object("bean", Keypoint("stem", 0.5 * w, 0.5 * h), [Keypoint("leaf", 0.25 * w, 0.7 * h), Keypoint("leaf", 1.0, 1.0)],
                                                    Box(0.3 * w, 0.3 * h, 0.7 * w, 0.8 * h)),
                                             Object("maize", Keypoint("stem", w - 2.0, 3.0), [])]) for i, (h, w) in enumerate(shapes)]
    aug = TrainAugmentation(Namespace(width=W, height=H, no_augmentation=False, device=torch.device(DEV), aug_perspective=0.5, aug_rotate=20.0,
                                      aug_scale=0.2))
    torch.manual_seed(21)
    flips, (words, factors) = aug.draws_for(n)                                          # the draws the call below makes, in its order
    warps = aug.affine_draws_for(n)
    quads = aug.perspective_draws_for(n)
    torch.manual_seed(21)
    out, anns = aug(imgs, make_anns())
    assert any(q is None for q in quads) and any(q is not None for q in quads) and warps is not None
    frame = [(0.0, 0.0), (float(W), 0.0), (float(W), float(H)), (0.0, float(H))]
    want_anns = make_anns()
    for i in range(n):
        inv6 = affine_inverse_matrix(size, warps[i][0], warps[i][1], warps[i][2:])
        fwd6 = affine_forward_matrix(size, warps[i][0], warps[i][1], warps[i][2:])
        row = compose_affine_perspective(inv6, IDENTITY if quads[i] is None else perspective_coeffs(frame, quads[i]))
        resized = np.asarray(Image.fromarray(imgs[i]).resize(size, Image.BILINEAR)).copy()
        order = [(words[i] >> (2 * k)) & 3 for k in range(4)]
        want = _finish(pil_perspective(resized, row), flips[i], (order, *factors[i], ((words[i] >> 8) & 255,)))
        assert torch.equal(out[i].cpu(), want), f"image {i}: {(out[i].cpu() != want).sum().item()} values differ"
        ann = want_anns[i]
        ann.resize((shapes[i][1], shapes[i][0]), size)
        if quads[i] is None:
            affine_annotation(ann, fwd6, size)
        else:
            perspective_annotation(ann, perspective_coeffs(quads[i], frame), size, affine_forward=fwd6)
        if flips[i] & 1:
            hflip_annotation(ann, size)
        if flips[i] & 2:
            vflip_annotation(ann, size)
        clip_annotation(ann, size)
        assert _rows(anns[i]) == _rows(ann), i
    assert sum(len(a.objects) for a in anns) >= n                                       # the centre objects stay


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
                "-e", "1", "--steps", "2", "--decode_workers", "2", "--aug_perspective", "0.3"] + extra)
    monkeypatch.setattr(T.Trainer, "train", orig)
    return trainers[0], capsys.readouterr().out


def _epoch_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("epoch 0:")]
    assert len(lines) == 1 and "(2 steps)" in lines[0], out
    losses = [float(v) for v in re.findall(r"(?:total|hm|offset|embedding) (\S+)", lines[0])]
    assert len(losses) == 4 and np.isfinite(losses).all() and losses[0] > 0, lines
    return lines[0]


@pytest.mark.parametrize("extra", [[], ["--cache_images", "0.5"], ["--keep_aspect"], ["--train_tiles", "2x2", "--tile_overlap", "32"]],
                         ids=["plain", "cache_images", "keep_aspect", "train_tiles"])
def test_train_cli_with_aug_perspective(golden_dir, tmp_path, monkeypatch, capsys, extra):
    """Two steps of `train --aug_perspective 0.3` from a PNG + JSON directory, alone and with the other sources and geometries: finite losses."""
    from tests.helpers import write_evaluate16_dir
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr, out = _train_run(tmp_path, "run", extra, monkeypatch, capsys)
    _epoch_line(out)
    assert tr.augment.perspective == 0.3 and torch.isfinite(tr.net.flat_params).all()
