"""Sensor noise on the GPU (sd_noise_u8: k_noise_u8; sd_preprocess_images_noise / _list_noise) byte for byte against tests/noise_ref.py,
which tests/test_noise_cpu.py pins to Philox's known-answer vectors and to a fresh half table: the stand-alone stage over sizes from one
pixel to several blocks and over constant, ramp and random content, independence of the batch geometry, in place, unaligned views, garbage
rows, the refusals, the chain forms against the hand composition of the existing entry points with the blur in front and the JPEG round trip
and the tone stage behind, a null table against the tone form, `TrainAugmentation` with the flags against Pillow's chain, and `train`."""
import functools
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.noise_ref import KINDS, MAX_A, MAX_B, noise_image, noise_ref, rows_of

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (height, width): one pixel; 15 bytes (the tail path only); a few chunks and a tail; whole chunks only; an odd byte count whose later
# images of a batch are not 16-byte aligned; and 99,369 bytes = four blocks of 32 KB with a tail of 9 bytes
SHAPES = [(1, 1), (1, 5), (3, 7), (16, 16), (37, 53), (181, 183)]
DRAWS = [(11, 12, 0.0, 0.0), (0xDEADBEEF, 42, 4.0, 0.0), (7, 0xFFFFFFFF, 0.0, 0.5), (123, 456, 32.0, 2.0)]   # off, read, shot, both at their maxima
PERM = [2, 0, 3, 1]


def _rows(draws=DRAWS):
    from structuredetector_amd.data import noise_rows
    return noise_rows(draws)


@functools.lru_cache(maxsize=None)
def _stage_case(shape, kind):
    """Four images of one kind and what the reference makes of them under the four rows: computed once, read only."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w + 7 * KINDS.index(kind))
    imgs = np.stack([noise_image(kind, h, w, rng) for _ in DRAWS])
    want = np.stack([noise_ref(a, r) for a, r in zip(imgs, rows_of(DRAWS))])
    imgs.setflags(write=False); want.setflags(write=False)
    return imgs, want


def _differences(got, want, what):
    for b in range(len(want)):
        bad = got[b] != want[b]
        assert not bad.any(), f"{what} image {b}: {bad.sum()} bytes differ, first at {np.argwhere(bad)[0].tolist()}"


def test_the_shapes_cover_the_paths():
    assert (181 * 183 * 3) % 16 != 0 and 181 * 183 * 3 > 3 * 32768 and 1 * 5 * 3 < 16 and (16 * 16 * 3) % 16 == 0 and (37 * 53 * 3) % 16 != 0
    assert [[v & 0xFFFFFFFF for v in r] for r in _rows()] == rows_of(DRAWS) == [[11, 12, 0, 0], [0xDEADBEEF, 42, 16 << 16, 0],
                                                                                  [7, 0xFFFFFFFF, 0, 32768], [123, 456, MAX_A, MAX_B]]


@pytest.mark.parametrize("kind", KINDS)
def test_sd_noise_u8_matches_the_reference_bytewise(kind):
    from structuredetector_amd.data import noise_images
    rows = _rows()
    for shape in SHAPES:
        imgs, want = _stage_case(shape, kind)
        x = torch.tensor(imgs, device=DEV)
        got = noise_images(x, rows).cpu().numpy()
        assert np.array_equal(x.cpu().numpy(), imgs)                 # the input is read only
        _differences(got, want, (kind, shape))
        assert np.array_equal(got[0], imgs[0])                       # the off image is untouched
        if shape[0] * shape[1] >= 256:
            assert all((want[b] != imgs[b]).any() for b in (1, 3)), (kind, shape)
            assert (want[2] != imgs[2]).any() or kind == "zeros"     # shot noise has nothing to add to black
        # the same rows in another order: a block reads its own image's row
        again = noise_images(torch.tensor(imgs[PERM], device=DEV), [rows[i] for i in PERM]).cpu().numpy()
        assert np.array_equal(again, want[PERM]), (kind, shape)


def test_the_bytes_do_not_depend_on_the_batch_geometry():
    """The same image and row alone in a call and at position 2 of 3 (where the image is not 16-byte aligned): the same bytes."""
    from structuredetector_amd.data import noise_images
    rows = _rows()
    for shape in ((37, 53), (181, 183)):
        imgs, want = _stage_case(shape, "ramp")
        assert imgs[0].size % 16 != 0
        for b in (1, 2, 3):
            alone = noise_images(torch.tensor(imgs[b:b + 1], device=DEV), [rows[b]]).cpu().numpy()[0]
            others = [(b + 1) % 4, (b + 2) % 4]
            third = noise_images(torch.tensor(imgs[others + [b]], device=DEV), [rows[i] for i in others + [b]]).cpu().numpy()[2]
            assert np.array_equal(alone, want[b]) and np.array_equal(third, want[b]), (shape, b)


def _raw_call(src_ptr, dst_ptr, B, H, W, table):
    from structuredetector_amd import _lib as L
    lib = L.lib()
    return lib.sd_noise_u8(src_ptr, dst_ptr, B, H, W, table.data_ptr() if table is not None else 0, L.stream()), lib


@pytest.mark.parametrize("kind", ["ramp", "random"])
def test_in_place_gives_the_same_bytes(kind):
    for shape in ((37, 53), (181, 183)):
        imgs, want = _stage_case(shape, kind)
        x = torch.tensor(imgs, device=DEV)
        table = torch.tensor(np.asarray(_rows(), dtype=np.int32), device=DEV)
        code, _ = _raw_call(x.data_ptr(), x.data_ptr(), *imgs.shape[:3], table)
        assert code == 0
        assert np.array_equal(x.cpu().numpy(), want)


def test_sd_noise_u8_on_views_that_are_not_16_byte_aligned():
    """Base addresses 1, 2 and 3 bytes (and more) past a 16-byte boundary, equal for in and out and different, with a width that leaves
    every later image of the batch unaligned too: the same bytes, and nothing in front of or behind the images is written."""
    imgs, want = _stage_case((37, 53), "random")
    B, H, W = imgs.shape[:3]
    n = imgs.size
    table = torch.tensor(np.asarray(_rows(), dtype=np.int32), device=DEV)
    flat = torch.tensor(imgs, device=DEV).reshape(-1)
    for a, o in ((1, 1), (2, 2), (3, 3), (1, 0), (0, 3), (5, 9), (15, 15), (16, 16)):
        arena_in = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
        arena_in[a:a + n].copy_(flat)
        arena_out = torch.full((n + 64,), 7, dtype=torch.uint8, device=DEV)
        assert arena_in.data_ptr() % 16 == 0 and arena_out.data_ptr() % 16 == 0
        code, _ = _raw_call(arena_in.data_ptr() + a, arena_out.data_ptr() + o, B, H, W, table)
        assert code == 0
        out = arena_out.cpu().numpy()
        assert np.array_equal(out[o:o + n].reshape(imgs.shape), want), (a, o)
        assert (out[:o] == 7).all() and (out[o + n:] == 7).all()     # nothing outside the images is written
        code, _ = _raw_call(arena_in.data_ptr() + a, arena_in.data_ptr() + a, B, H, W, table)       # in place, unaligned
        assert code == 0
        back = arena_in.cpu().numpy()
        assert np.array_equal(back[a:a + n].reshape(imgs.shape), want), a
        assert not back[:a].any() and not back[a + n:].any()


def test_garbage_rows_give_the_clamped_reference():
    """All-ones, negative, and `a` alone beyond the clamp: the variance words are read as uint32 and clamped; the keys are any 32 bits."""
    from structuredetector_amd.data import noise_images
    rng = np.random.default_rng(8)
    h, w = 37, 53
    rows = [[-1, -1, -1, -1], [5, 6, -2 ** 31, -2 ** 31], [5, 6, MAX_A + 1, 0], [5, 6, 2 ** 31 - 1, 3], [-2 ** 31, 2 ** 31 - 1, 0, MAX_B + 1],
            [9, 9, -7, 0], [9, 9, 0, -7], [2 ** 31 - 1, -2 ** 31, 0, 0]]
    imgs = np.stack([noise_image("ramp", h, w, rng) for _ in rows])
    want = np.stack([noise_ref(a, r) for a, r in zip(imgs, rows)])
    assert np.array_equal(want[0], noise_ref(imgs[0], [0xFFFFFFFF, 0xFFFFFFFF, MAX_A, MAX_B]))
    assert np.array_equal(want[2], noise_ref(imgs[2], [5, 6, MAX_A, 0])) and np.array_equal(want[7], imgs[7])
    assert all((want[b] != imgs[b]).any() for b in range(7))
    got = noise_images(torch.tensor(imgs, device=DEV), rows).cpu().numpy()
    _differences(got, want, "garbage")


def test_bad_calls_are_refused_before_any_launch():
    from structuredetector_amd import _lib as L
    H, W = 9, 20
    x = torch.full((2, H, W, 3), 9, dtype=torch.uint8, device=DEV)
    out = torch.full((2, H, W, 3), 3, dtype=torch.uint8, device=DEV)
    table = torch.tensor(np.asarray(_rows()[1:3], dtype=np.int32), device=DEV)
    cases = [(dict(table=None), "null"), (dict(src=0), "null"), (dict(dst=0), "null"), (dict(dst=x.data_ptr() + 3 * W), "overlap"),
             (dict(dst=x.data_ptr() - 1), "overlap"), (dict(B=65536), "65535"), (dict(H=0), "bad shape"), (dict(B=0), "bad shape")]
    for kw, text in cases:
        code, lib = _raw_call(kw.get("src", x.data_ptr()), kw.get("dst", out.data_ptr()), kw.get("B", 2), kw.get("H", H), W, kw.get("table", table))
        assert code == -1, (kw, code)                                # SD_ERR_INVALID
        msg = lib.sd_last_error().decode()
        assert "sd_noise_u8" in msg and text in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (out == 3).all() and (x == 9).all()                       # no launch was left behind
    from structuredetector_amd.data import noise_images
    with pytest.raises(L.SdError, match="one row"):
        noise_images(x, _rows()[:1])
    with pytest.raises(L.SdError, match="uint8"):
        noise_images(x.float(), _rows()[:2])


# ---- the chain forms -------------------------------------------------------------------------------------------------------------
def _behind_tables(n_pixels):
    from structuredetector_amd.data import jpeg_rows, tone_rows
    from tests.tone_ref import AUTOCONTRAST, COPY, EQUALIZE
    return dict(jpeg=jpeg_rows([50, 0, 90, 10]), tone=tone_rows([(COPY, 0.0), (EQUALIZE, 0.0), (AUTOCONTRAST, 5.0), (AUTOCONTRAST, 0.0)], n_pixels))


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_chain_forms_equal_the_hand_composition(geometry):
    """The blur form up to its 8-bit frame (its bytes read back through an identity tail), `noise_images` on those bytes, then the existing
    JPEG / tone / jitter / flips / normalise on the result (an identity resize): the packed and the list form of the noise chain give that
    tensor bit for bit, for the stage sets of the blur's test -- with the noise table alone (every other table null), with the blur in front,
    and with the blur in front and the JPEG round trip and the tone stage behind, where a stage on the wrong side would show."""
    from structuredetector_amd.data import blur_box_params, noise_images, preprocess_image_list, preprocess_images
    from tests.test_gpu_blur import NB, OUT, RADII, SRC, _bytes, _geometry, _sources, _stage_sets, _table
    x = torch.tensor(_sources(), device=DEV)
    arena, table = _table()
    geom = _geometry(geometry)
    rows = _rows()
    blur = dict(blur=[blur_box_params(r) for r in RADII])
    for name, front, behind in _stage_sets():
        for before, after in (({}, {}), (blur, {}), (blur, _behind_tables(OUT[0] * OUT[1]))):
            tag = f"{geometry} {name} {sorted(before)} {sorted(after)}"
            head = preprocess_images(x, OUT, **geom, **front, **before)                    # the blur form (or the existing entry point)
            u8 = _bytes(head)
            assert torch.equal(preprocess_images(torch.tensor(u8, device=DEV), OUT), head), tag         # the bytes, and the identity resize
            noised = noise_images(torch.tensor(u8, device=DEV), rows)
            host = noised.cpu().numpy()
            assert np.array_equal(host, np.stack([noise_ref(u8[b], rows[b]) for b in range(NB)])), tag
            assert np.array_equal(host[0], u8[0]) and all((host[b] != u8[b]).any() for b in (1, 2, 3)), tag
            want = preprocess_images(noised, OUT, **after, **behind)
            if after:                                                # the other order is another tensor: the test can tell the sides apart
                swapped = noise_images(torch.tensor(_bytes(preprocess_images(torch.tensor(u8, device=DEV), OUT, **after)), device=DEV), rows)
                assert not torch.equal(preprocess_images(swapped, OUT, **behind), want), tag
            for form, got in (("packed", preprocess_images(x, OUT, **geom, **front, **before, **after, **behind, noise=rows)),
                              ("list", preprocess_image_list(table, SRC[0], SRC[1], OUT, **geom, **front, **before, **after, **behind, noise=rows))):
                if "jitter" not in behind:                           # the bytes themselves
                    bad = (_bytes(got) != _bytes(want)).sum()
                    assert bad == 0, f"{form} {tag}: {bad} bytes differ"
                assert torch.equal(got, want), f"{form} {tag}: {(got != want).sum().item()} values differ"
    del arena


def test_the_noise_comes_behind_the_blur():
    """Noise, then blur is another image than blur, then noise: the chain gives the second."""
    from structuredetector_amd.data import blur_box_params, blur_images, noise_images, preprocess_images
    from tests.test_gpu_blur import OUT, RADII, _bytes, _sources
    x = torch.tensor(_sources(), device=DEV)
    rows, boxes = _rows(), [blur_box_params(r) for r in RADII]
    u8 = torch.tensor(_bytes(preprocess_images(x, OUT)), device=DEV)
    right = preprocess_images(noise_images(blur_images(u8, boxes), rows), OUT)
    wrong = preprocess_images(blur_images(noise_images(u8, rows), boxes), OUT)
    got = preprocess_images(x, OUT, blur=boxes, noise=rows)
    assert torch.equal(got, right) and not torch.equal(got, wrong)


def test_the_chain_has_no_size_rule_of_its_own():
    """An odd frame (JPEG would refuse it) through the noise form, against the hand composition."""
    from structuredetector_amd.data import noise_images, preprocess_images
    from tests.test_gpu_blur import _bytes, _sources
    x = torch.tensor(_sources(), device=DEV)
    out = (31, 27)
    rows = _rows()
    head = preprocess_images(x, out)
    want = preprocess_images(noise_images(torch.tensor(_bytes(head), device=DEV), rows), out)
    assert torch.equal(preprocess_images(x, out, noise=rows), want) and not torch.equal(want, head)


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_a_null_table_is_the_tone_form_bit_for_bit(geometry):
    from structuredetector_amd.data import blur_box_params, preprocess_image_list, preprocess_images
    from structuredetector_amd.data.augment import _MEAN, _STD
    from tests.helpers import call_legacy_preprocess_form as _preprocess_blur
    from tests.test_gpu_blur import NB, OUT, RADII, SRC, _geometry, _sources, _stage_sets, _table
    x = torch.tensor(_sources(), device=DEV)
    arena, table = _table()
    geom = _geometry(geometry)
    tables = _behind_tables(OUT[0] * OUT[1])
    for name, front, behind in _stage_sets():
        for extra in ({}, dict(tone=tables["tone"]), dict(**tables, blur=[blur_box_params(r) for r in RADII])):
            kw = dict(flips=None, jitter=None, affine=None, mosaic=None, window=None, letterbox=None, blur=None, persp=None, jpeg=None, tone=None)
            kw.update(geom); kw.update(front); kw.update(behind); kw.update(extra)
            stages = {k: v for k, v in kw.items() if v is not None}
            args = (NB, SRC[0], SRC[1], OUT, kw["flips"], _MEAN, _STD, kw["jitter"], kw["affine"], kw["mosaic"], kw["window"], kw["letterbox"], kw["blur"],
                    x.device, kw["persp"], kw["jpeg"], kw["tone"], None)
            want = preprocess_images(x, OUT, **stages)
            assert torch.equal(_preprocess_blur("sd_preprocess_images_noise", x.data_ptr(), *args), want), (name, sorted(extra))
            want = preprocess_image_list(table, SRC[0], SRC[1], OUT, **stages)
            assert torch.equal(_preprocess_blur("sd_preprocess_images_list_noise", table.data_ptr(), *args), want), (name, sorted(extra))
    del arena


def test_chain_rejects_what_it_cannot_do():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import jpeg_rows, preprocess_images
    x = torch.zeros((1, 20, 20, 3), dtype=torch.uint8, device=DEV)
    one = _rows()[1:2]
    with pytest.raises(L.SdError, match="one row"):
        preprocess_images(x, (16, 16), noise=one * 2)
    with pytest.raises(L.SdError, match="16 x 16 MCUs"):             # JPEG's rule holds when its table is set too
        preprocess_images(x, (24, 16), noise=one, jpeg=jpeg_rows([50]))
    with pytest.raises(L.SdError, match="do not combine"):
        preprocess_images(x, (16, 16), noise=one, persp=[[1.0, 0, 0, 0, 1.0, 0, 0, 0]], affine=[[1.0, 0, 0, 0, 1.0, 0]])


# ---- the augmentation class and the CLI ------------------------------------------------------------------------------------------
def _pillow_chain(img, size, r, row, jit, hflip, vflip):
    """Resize -> GaussianBlur -> noise_ref -> ColorJitter -> flips -> to_tensor -> Normalize, every other image operation Pillow's own."""
    from PIL import Image, ImageFilter
    from tests.test_gpu_pipeline import MEAN, STD, pil_color_jitter
    im = Image.fromarray(img).resize(size, Image.BILINEAR)
    if r > 0:
        im = im.filter(ImageFilter.GaussianBlur(r))
    if row is not None:
        im = Image.fromarray(noise_ref(np.asarray(im), row))
    im = pil_color_jitter(im, *jit)
    if hflip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if vflip:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    return torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).to(torch.float32).div(255).sub(MEAN).div(STD)


def test_train_augmentation_with_the_flags_equals_the_pillow_chain():
    from structuredetector_amd.data import TrainAugmentation, noise_rows
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    size, n = (96, 64), 6
    rng = np.random.default_rng(9)
    imgs = [rng.integers(0, 256, (60, 80, 3), dtype=np.uint8) for _ in range(n)]
    make_anns = lambda: [ImageAnnotation(f"{i}.png", [Object("bean", Keypoint("stem", 10.0 * i + 1, 5.0 * i + 2), [])]) for i in range(n)]
    common = dict(width=size[0], height=size[1], no_augmentation=False, device=torch.device(DEV), aug_blur=2.0)
    outs = {}
    for on in (True, False):
        aug = TrainAugmentation(Namespace(**common, **(dict(aug_noise=6.0, aug_noise_shot=0.5) if on else {})))
        torch.manual_seed(21)
        flips, (words, factors) = aug.draws_for(n)                   # the draws the call below makes, in its order
        radii = aug.blur_draws_for(n)
        draws = aug.noise_draws_for(n)
        torch.manual_seed(21)
        out, anns = aug(imgs, make_anns())
        if on:
            assert any(d[2] > 0 for d in draws) and any(d[2] == 0 and d[3] == 0 for d in draws) and all(d[2] <= 6.0 and d[3] <= 0.5 for d in draws)
            rows = noise_rows(draws)
        else:
            assert draws is None
        for i in range(n):
            order = [(words[i] >> (2 * k)) & 3 for k in range(4)]
            jit = (order, *factors[i], ((words[i] >> 8) & 255,))
            want = _pillow_chain(imgs[i], size, radii[i], rows[i] if on else None, jit, bool(flips[i] & 1), bool(flips[i] & 2))
            assert torch.equal(out[i].cpu(), want), f"{'on' if on else 'off'} image {i}: {(out[i].cpu() != want).sum().item()} values differ"
        outs[on] = (out.cpu(), [(a.objects[0].x, a.objects[0].y) for a in anns])
    assert outs[True][1] == outs[False][1]                           # photometric: the annotations are those of the plain chain
    assert not torch.equal(outs[True][0], outs[False][0])


def _train_args(tmp_path, source):
    return source + ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "-b", "4", "-e", "1", "--steps", "2",
                     "--decode_workers", "2", "--aug_noise", "6", "--aug_noise_shot", "0.5"]


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
    train.main(_train_args(tmp_path, ["--train_dir", str(tmp_path / "train")]) + extra)
    monkeypatch.setattr(T.Trainer, "train", orig)
    return trainers[0], capsys.readouterr().out


def test_train_cli_with_the_flags_with_and_without_the_image_cache(golden_dir, tmp_path, monkeypatch, capsys):
    """Two steps of `train --aug_noise 6 --aug_noise_shot 0.5` from a PNG + JSON directory: finite losses, the same twice from the same
    seed, and identical with and without --cache_images (the packed and the pointer-list form of the chain)."""
    from tests.helpers import write_evaluate16_dir
    from tests.test_gpu_blur import _epoch_line
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr_a, out_a = _train_run(tmp_path, "plain", [], monkeypatch, capsys)
    tr_b, out_b = _train_run(tmp_path, "cached", ["--cache_images", "0.5"], monkeypatch, capsys)
    tr_c, out_c = _train_run(tmp_path, "again", [], monkeypatch, capsys)
    assert tr_a.cache is None and tr_b.cache is not None
    assert (tr_a.augment.noise, tr_a.augment.noise_shot) == (6.0, 0.5)
    assert _epoch_line(out_a) == _epoch_line(out_b) == _epoch_line(out_c)
    assert torch.isfinite(tr_a.net.flat_params).all() and torch.equal(tr_a.net.flat_params, tr_b.net.flat_params)
    assert torch.equal(tr_a.net.flat_params, tr_c.net.flat_params)


@pytest.mark.parametrize("extra", [["--keep_aspect"], ["--train_tiles", "2x2", "--tile_overlap", "32"],
                                   ["--aug_jpeg", "40", "--aug_blur", "2", "--aug_equalize", "0.4", "--aug_autocontrast", "0.6"],
                                   ["--aug_rotate", "10", "--aug_mosaic", "0.5", "--aug_perspective", "0.3"]],
                         ids=["keep_aspect", "train_tiles", "blur_jpeg_tone", "warps"])
def test_train_cli_with_the_flags_beside_the_other_flags(golden_dir, tmp_path, monkeypatch, capsys, extra):
    from tests.helpers import write_evaluate16_dir
    from tests.test_gpu_blur import _epoch_line
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr, out = _train_run(tmp_path, "run", extra, monkeypatch, capsys)
    _epoch_line(out)
    assert tr.augment.noise == 6.0 and torch.isfinite(tr.net.flat_params).all()


def test_train_cli_refuses_the_flags_with_synthetic(tmp_path, monkeypatch):
    from structuredetector_amd.cli import train
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="'aug_noise' / 'aug_noise_shot' work on source images: they need --train_dir, not --synthetic"):
        train.main(_train_args(tmp_path, ["--synthetic", "8"]))
