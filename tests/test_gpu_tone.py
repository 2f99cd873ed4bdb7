"""Histogram tone curves on the GPU (sd_tone_u8: k_tone_hist, k_tone_lut, k_tone_apply; sd_preprocess_images_tone / _list_tone) byte for
byte against Pillow's ImageOps.equalize / ImageOps.autocontrast and against tests/tone_ref.py, which tests/test_tone_cpu.py pins to Pillow:
the stand-alone stage over sizes from one pixel to several histogram strips and over flat and noisy content, in place, unaligned views,
every (lo, hi) pair of the double-precision stretch, garbage tables, the refusals, the chain forms against the hand composition of the
existing entry points, a null table against the JPEG form, `TrainAugmentation` with the flags against Pillow's own chain, and `train`."""
import functools
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.tone_ref import AUTOCONTRAST, COPY, EQUALIZE, KINDS, cut_of, pillow_tone, tone_image, tone_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _strip_pixels():
    from structuredetector_amd.data.augment import TONE_STRIP_PIXELS
    return TONE_STRIP_PIXELS


def _shapes():
    """(height, width): one pixel; 15 bytes (the tail path only); a few chunks; whole chunks; an odd byte count; and more than 8 histogram
    strips an image, with an odd byte count (several blocks add into one histogram)."""
    side = int(np.sqrt(8 * _strip_pixels())) + 1
    return [(1, 1), (1, 5), (3, 7), (16, 16), (37, 53), (side, side)]


MODES = [EQUALIZE, COPY, AUTOCONTRAST]                               # mixed in one call: the slots of neighbouring images must not leak
CUTOFF = 2.0


def _rows(n_pixels, cutoff=CUTOFF):
    from structuredetector_amd.data import tone_rows
    return tone_rows([(EQUALIZE, 0.0), (COPY, 0.0), (AUTOCONTRAST, cutoff)], n_pixels)


@functools.lru_cache(maxsize=None)
def _stage_case(shape, kind):
    """Three images of one kind, their rows and what Pillow makes of them: computed once, read only."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w + 7 * KINDS.index(kind))
    imgs = np.stack([tone_image(kind, h, w, rng) for _ in MODES])
    rows = _rows(h * w)
    want = np.stack([pillow_tone(a, m, CUTOFF) for a, m in zip(imgs, MODES)])
    imgs.setflags(write=False); want.setflags(write=False)
    return imgs, rows, want


def _differences(got, want, what):
    for b in range(len(want)):
        bad = got[b] != want[b]
        assert not bad.any(), f"{what} image {b}: {bad.sum()} bytes differ, first at {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("kind", KINDS)
def test_sd_tone_u8_matches_pillow_bytewise(kind):
    from structuredetector_amd.data import tone_images
    changed = 0
    for shape in _shapes():
        imgs, rows, want = _stage_case(shape, kind)
        cut = cut_of(shape[0] * shape[1], CUTOFF)
        assert rows == [[2, 0, 0, 0], [0, 0, 0, 0], [1, cut, cut, 0]]
        assert np.array_equal(want, np.stack([tone_ref(a, r) for a, r in zip(imgs, rows)]))
        x = torch.tensor(imgs, device=DEV)
        got = tone_images(x, rows).cpu().numpy()
        assert np.array_equal(x.cpu().numpy(), imgs)                 # the input is read only
        _differences(got, want, (kind, shape))
        assert np.array_equal(got[1], imgs[1])                       # the mode-0 image is untouched
        changed += int((want != imgs).any())
        # the same rows in another order: a block reads its own image's row and its own histogram
        perm = [2, 0, 1]
        again = tone_images(torch.tensor(imgs[perm], device=DEV), [rows[i] for i in perm]).cpu().numpy()
        assert np.array_equal(again, want[perm]), (kind, shape)
    assert changed >= (0 if kind == "constant" else 3)


def test_the_largest_shape_spans_more_than_eight_histogram_strips():
    h, w = _shapes()[-1]
    assert h * w >= 8 * _strip_pixels() and (h * w * 3) % 16 != 0


def _raw_call(src_ptr, dst_ptr, B, H, W, table, ws=None, ws_bytes=None):
    from structuredetector_amd import _lib as L
    lib = L.lib()
    if ws is None:
        ws = L.workspace(lib.sd_tone_workspace_bytes(B), torch.device(DEV, torch.cuda.current_device()))
    table_ptr = table.data_ptr() if table is not None else 0
    return lib.sd_tone_u8(src_ptr, dst_ptr, B, H, W, table_ptr, ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, L.stream()), lib


@pytest.mark.parametrize("kind", ["noise", "mostly_one"])
def test_in_place_gives_the_same_bytes(kind):
    for shape in (_shapes()[4], _shapes()[-1]):
        imgs, rows, want = _stage_case(shape, kind)
        x = torch.tensor(imgs, device=DEV)
        table = torch.tensor(np.asarray(rows, dtype=np.int32), device=DEV)
        code, _ = _raw_call(x.data_ptr(), x.data_ptr(), *imgs.shape[:3], table)
        assert code == 0
        assert np.array_equal(x.cpu().numpy(), want)


def test_sd_tone_u8_on_views_that_are_not_16_byte_aligned():
    """Base addresses at every kind of offset from a 16-byte boundary, equal for in and out (the chunk path behind a head) and different
    (the byte path): the same bytes, and nothing outside the images is written."""
    imgs, rows, want = _stage_case((37, 53), "narrow")
    B, H, W = imgs.shape[:3]
    n = imgs.size
    table = torch.tensor(np.asarray(rows, dtype=np.int32), device=DEV)
    flat = torch.tensor(imgs, device=DEV).reshape(-1)
    for a, o in ((5, 5), (5, 3), (4, 8), (0, 9), (15, 15), (1, 17)):
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


def test_every_lo_hi_pair_of_the_stretch():
    """B = 10,880 images of 1 x 256: channel c of image b carries pair p = 3 b + c of the 32,640 with lo < hi, and its pixels are
    lo + (x mod (hi - lo + 1)), so every table entry in [lo, hi] is read.  A contracted multiply-add in the kernel differs here."""
    from structuredetector_amd.data import tone_images
    pairs = np.asarray([(lo, hi) for lo in range(255) for hi in range(lo + 1, 256)])
    assert len(pairs) == 32640 == 3 * 10880
    lo, hi = pairs[:, 0].reshape(-1, 3), pairs[:, 1].reshape(-1, 3)
    x = np.arange(256).reshape(1, 256, 1)
    imgs = (lo[:, None, :] + x % (hi - lo + 1)[:, None, :]).astype(np.uint8).reshape(-1, 1, 256, 3)
    assert all(imgs[b, 0, :, c].min() == lo[b, c] and imgs[b, 0, :, c].max() == hi[b, c] for b in (0, 5000, 10879) for c in range(3))
    rows = [[AUTOCONTRAST, 0, 0, 0]] * len(imgs)
    want = np.stack([tone_ref(a, rows[0]) for a in imgs])
    integer = ((imgs.astype(np.int64) - lo[:, None, None, :]) * 255) // (hi - lo)[:, None, None, :]
    assert (want != integer).any()                                   # the exact quotient is not the answer
    got = tone_images(torch.tensor(imgs, device=DEV), rows).cpu().numpy()
    bad = (got != want).reshape(len(imgs), -1).any(axis=1)
    assert not bad.any(), f"{bad.sum()} images differ, first {int(np.flatnonzero(bad)[0])}"


def test_garbage_rows_give_defined_bytes():
    """Modes other than 1 and 2 copy; cuts are clamped to [0, n]; the fourth entry is ignored."""
    from structuredetector_amd.data import tone_images
    rng = np.random.default_rng(8)
    h, w = 37, 53
    rows = [[7, 3, 3, 0], [-1, 0, 0, 0], [AUTOCONTRAST, -5, -5, 0], [AUTOCONTRAST, 2 ** 31 - 1, 0, 0], [AUTOCONTRAST, 0, 2 ** 31 - 1, 9],
            [AUTOCONTRAST, -2 ** 31, 2 ** 31 - 1, -1], [EQUALIZE, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1], [3, -2 ** 31, -2 ** 31, 0],
            [2 ** 31 - 1, 1, 1, 1], [AUTOCONTRAST, h * w, 0, 0], [AUTOCONTRAST, h * w - 1, 0, 0]]
    imgs = np.stack([tone_image("narrow", h, w, rng) for _ in rows])
    want = np.stack([tone_ref(a, r) for a, r in zip(imgs, rows)])
    for b in (0, 1, 3, 4, 5, 7, 8, 9):
        assert np.array_equal(want[b], imgs[b])
    assert np.array_equal(want[2], pillow_tone(imgs[2], AUTOCONTRAST, 0)) and np.array_equal(want[6], pillow_tone(imgs[6], EQUALIZE))
    assert (want[2] != imgs[2]).any() and (want[6] != imgs[6]).any()
    got = tone_images(torch.tensor(imgs, device=DEV), rows).cpu().numpy()
    _differences(got, want, "garbage")


def test_bad_calls_are_refused_before_any_launch():
    from structuredetector_amd import _lib as L
    H, W = 9, 20
    x = torch.full((2, H, W, 3), 9, dtype=torch.uint8, device=DEV)
    out = torch.full((2, H, W, 3), 3, dtype=torch.uint8, device=DEV)
    table = torch.tensor(np.asarray([[2, 0, 0, 0], [1, 1, 1, 0]], dtype=np.int32), device=DEV)
    dev = torch.device(DEV, torch.cuda.current_device())
    full = L.lib().sd_tone_workspace_bytes(2)
    invalid, too_small = -1, -2                                      # SD_ERR_INVALID, SD_ERR_WORKSPACE
    cases = [(dict(table=None), invalid, "null"), (dict(src=0), invalid, "null"), (dict(dst=0), invalid, "null"),
             (dict(ws_bytes=full - 1), too_small, f"workspace {full - 1} < {full}"), (dict(dst=x.data_ptr() + 3 * W), invalid, "overlap"),
             (dict(dst=x.data_ptr() - 1), invalid, "overlap"), (dict(B=65536), invalid, "65535"), (dict(H=0), invalid, "bad shape")]
    for kw, expected, text in cases:
        code, lib = _raw_call(kw.get("src", x.data_ptr()), kw.get("dst", out.data_ptr()), kw.get("B", 2), kw.get("H", H), W, kw.get("table", table),
                              L.workspace(full, dev), kw.get("ws_bytes"))
        assert code == expected, (kw, code)
        msg = lib.sd_last_error().decode()
        assert "sd_tone_u8" in msg and text in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (out == 3).all() and (x == 9).all()                       # no launch was left behind
    from structuredetector_amd.data import tone_images
    with pytest.raises(L.SdError, match="one row"):
        tone_images(x, [[2, 0, 0, 0]])
    with pytest.raises(L.SdError, match="uint8"):
        tone_images(x.float(), [[2, 0, 0, 0]] * 2)


# ---- the chain forms -------------------------------------------------------------------------------------------------------------
def _chain_rows(n_pixels):
    from structuredetector_amd.data import tone_rows
    return tone_rows([(COPY, 0.0), (EQUALIZE, 0.0), (AUTOCONTRAST, 5.0), (AUTOCONTRAST, 0.0)], n_pixels)     # one image of the batch stays as it is


def _jpeg_rows():
    from structuredetector_amd.data import jpeg_rows
    return jpeg_rows([50, 0, 90, 10])


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_chain_forms_equal_the_hand_composition(geometry):
    """The JPEG form up to its 8-bit frame (its bytes read back through an identity tail), `tone_images` on those bytes, then the existing
    jitter / flips / normalise on the result (an identity resize): the packed and the list form of the tone chain give that tensor bit for
    bit, for the stage sets of the blur's test, with and without the JPEG table and the blur in front."""
    from structuredetector_amd.data import blur_box_params, preprocess_image_list, preprocess_images, tone_images
    from tests.test_gpu_blur import NB, OUT, RADII, SRC, _bytes, _geometry, _sources, _stage_sets, _table
    x = torch.tensor(_sources(), device=DEV)
    arena, table = _table()
    geom = _geometry(geometry)
    rows = _chain_rows(OUT[0] * OUT[1])
    for name, front, behind in _stage_sets():
        for extra in ({}, dict(jpeg=_jpeg_rows()), dict(jpeg=_jpeg_rows(), blur=[blur_box_params(r) for r in RADII])):
            tag = f"{geometry} {name} {sorted(extra)}"
            head = preprocess_images(x, OUT, **geom, **front, **extra)                     # the JPEG form (or the existing entry point)
            u8 = _bytes(head)
            assert torch.equal(preprocess_images(torch.tensor(u8, device=DEV), OUT), head), tag         # the bytes, and the identity resize
            toned = tone_images(torch.tensor(u8, device=DEV), rows)
            host = toned.cpu().numpy()
            assert np.array_equal(host, np.stack([tone_ref(u8[b], rows[b]) for b in range(NB)])), tag
            # (a frame that already spans 0 .. 255, as behind a coarse JPEG table, is autocontrast's fixed point: only "some" is asked of those)
            assert np.array_equal(host[0], u8[0]) and (host[1] != u8[1]).any() and (host[2:] != u8[2:]).any(), tag
            want = preprocess_images(toned, OUT, **behind)
            for form, got in (("packed", preprocess_images(x, OUT, **geom, **front, **extra, **behind, tone=rows)),
                              ("list", preprocess_image_list(table, SRC[0], SRC[1], OUT, **geom, **front, **extra, **behind, tone=rows))):
                if "jitter" not in behind:                           # the bytes themselves
                    bad = (_bytes(got) != _bytes(want)).sum()
                    assert bad == 0, f"{form} {tag}: {bad} bytes differ"
                assert torch.equal(got, want), f"{form} {tag}: {(got != want).sum().item()} values differ"
    del arena


def test_the_chain_has_no_size_rule_of_its_own():
    """An odd frame (JPEG would refuse it) through the tone form, against the hand composition."""
    from structuredetector_amd.data import preprocess_images, tone_images
    from tests.test_gpu_blur import _bytes, _sources
    x = torch.tensor(_sources(), device=DEV)
    out = (31, 27)
    rows = _chain_rows(31 * 27)
    head = preprocess_images(x, out)
    want = preprocess_images(tone_images(torch.tensor(_bytes(head), device=DEV), rows), out)
    assert torch.equal(preprocess_images(x, out, tone=rows), want) and not torch.equal(want, head)


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_a_null_table_is_the_jpeg_form_bit_for_bit(geometry):
    from structuredetector_amd.data import blur_box_params, preprocess_image_list, preprocess_images
    from structuredetector_amd.data.augment import _MEAN, _STD
    from tests.helpers import call_legacy_preprocess_form as _preprocess_blur
    from tests.test_gpu_blur import NB, OUT, RADII, SRC, _geometry, _sources, _stage_sets, _table
    x = torch.tensor(_sources(), device=DEV)
    arena, table = _table()
    geom = _geometry(geometry)
    for name, front, behind in _stage_sets():
        for extra in ({}, dict(jpeg=_jpeg_rows()), dict(jpeg=_jpeg_rows(), blur=[blur_box_params(r) for r in RADII])):
            kw = dict(flips=None, jitter=None, affine=None, mosaic=None, window=None, letterbox=None, blur=None, persp=None, jpeg=None)
            kw.update(geom); kw.update(front); kw.update(behind); kw.update(extra)
            stages = {k: v for k, v in kw.items() if v is not None}
            args = (NB, SRC[0], SRC[1], OUT, kw["flips"], _MEAN, _STD, kw["jitter"], kw["affine"], kw["mosaic"], kw["window"], kw["letterbox"], kw["blur"],
                    x.device, kw["persp"], kw["jpeg"], None)
            want = preprocess_images(x, OUT, **stages)
            assert torch.equal(_preprocess_blur("sd_preprocess_images_tone", x.data_ptr(), *args), want), (name, sorted(extra))
            want = preprocess_image_list(table, SRC[0], SRC[1], OUT, **stages)
            assert torch.equal(_preprocess_blur("sd_preprocess_images_list_tone", table.data_ptr(), *args), want), (name, sorted(extra))
    del arena


def test_chain_rejects_what_it_cannot_do():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import preprocess_images
    x = torch.zeros((1, 20, 20, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.SdError, match="one row"):
        preprocess_images(x, (16, 16), tone=[[2, 0, 0, 0]] * 2)
    with pytest.raises(L.SdError, match="16 x 16 MCUs"):             # JPEG's rule holds when its table is set too
        preprocess_images(x, (24, 16), tone=[[2, 0, 0, 0]], jpeg=_jpeg_rows()[:1])
    with pytest.raises(L.SdError, match="do not combine"):
        preprocess_images(x, (16, 16), tone=[[2, 0, 0, 0]], persp=[[1.0, 0, 0, 0, 1.0, 0, 0, 0]], affine=[[1.0, 0, 0, 0, 1.0, 0]])


# ---- the augmentation class and the CLI ------------------------------------------------------------------------------------------
def _pillow_chain(img, size, draw, jit, hflip, vflip):
    """Resize -> ImageOps.equalize / autocontrast -> ColorJitter -> flips -> to_tensor -> Normalize, every image operation Pillow's own."""
    from PIL import Image, ImageOps
    from tests.test_gpu_pipeline import MEAN, STD, pil_color_jitter
    im = Image.fromarray(img).resize(size, Image.BILINEAR)
    if draw[0] == EQUALIZE:
        im = ImageOps.equalize(im)
    elif draw[0] == AUTOCONTRAST:
        im = ImageOps.autocontrast(im, cutoff=draw[1])
    im = pil_color_jitter(im, *jit)
    if hflip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if vflip:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    return torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).to(torch.float32).div(255).sub(MEAN).div(STD)


def _golden_images(golden_dir, tmp_path, n):
    """The first n scenes of tests/golden/evaluate16.npz as the suite materialises them, dimmed into a part of the range so that both
    curves have something to do."""
    from PIL import Image
    from tests.helpers import write_evaluate16_dir
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "golden")
    imgs = [np.asarray(Image.open(tmp_path / "golden" / f"img_{i:02d}.png").convert("RGB")) for i in range(n)]
    return [(40 + a.astype(np.int32) * (100 + 10 * i) // 255).astype(np.uint8) for i, a in enumerate(imgs)]


@pytest.mark.parametrize("flags", [dict(aug_equalize=1.0), dict(aug_autocontrast=1.0, aug_autocontrast_cutoff=5.0),
                                   dict(aug_equalize=0.4, aug_autocontrast=0.5, aug_autocontrast_cutoff=40.0)],
                         ids=["equalize", "autocontrast", "mixed"])
def test_train_augmentation_with_the_flags_equals_the_pillow_chain(golden_dir, tmp_path, flags):
    from structuredetector_amd.data import TrainAugmentation
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    size, n = (96, 64), 6
    imgs = _golden_images(golden_dir, tmp_path, n)
    make_anns = lambda: [ImageAnnotation(f"{i}.png", [Object("bean", Keypoint("stem", 10.0 * i + 1, 5.0 * i + 2), [])]) for i in range(n)]
    common = dict(width=size[0], height=size[1], no_augmentation=False, device=torch.device(DEV))
    outs = {}
    for on in (True, False):
        aug = TrainAugmentation(Namespace(**common, **(flags if on else {})))
        torch.manual_seed(21)
        flips, (words, factors) = aug.draws_for(n)                   # the draws the call below makes, in its order
        draws = aug.tone_draws_for(n)
        torch.manual_seed(21)
        out, anns = aug(imgs, make_anns())
        if on:
            assert len({m for m, _ in draws}) == (1 if len(flags) < 3 else 3), draws
        else:
            assert draws is None
        for i in range(n):
            order = [(words[i] >> (2 * k)) & 3 for k in range(4)]
            jit = (order, *factors[i], ((words[i] >> 8) & 255,))
            want = _pillow_chain(imgs[i], size, draws[i] if draws else (COPY, 0.0), jit, bool(flips[i] & 1), bool(flips[i] & 2))
            assert torch.equal(out[i].cpu(), want), f"{flags if on else 'off'} image {i}: {(out[i].cpu() != want).sum().item()} values differ"
        outs[on] = (out.cpu(), [(a.objects[0].x, a.objects[0].y) for a in anns])
    assert outs[True][1] == outs[False][1]                           # photometric: the annotations are those of the plain chain
    assert not torch.equal(outs[True][0], outs[False][0])


def _train_args(tmp_path, source):
    return source + ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "-b", "4", "-e", "1", "--steps", "2",
                     "--decode_workers", "2", "--aug_equalize", "0.4", "--aug_autocontrast", "0.6", "--aug_autocontrast_cutoff", "5"]


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
    """Two steps of `train --aug_equalize --aug_autocontrast` from a PNG + JSON directory: finite losses, identical with and without
    --cache_images (the packed and the pointer-list form of the chain)."""
    from tests.helpers import write_evaluate16_dir
    from tests.test_gpu_blur import _epoch_line
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr_a, out_a = _train_run(tmp_path, "plain", [], monkeypatch, capsys)
    tr_b, out_b = _train_run(tmp_path, "cached", ["--cache_images", "0.5"], monkeypatch, capsys)
    assert tr_a.cache is None and tr_b.cache is not None
    assert (tr_a.augment.equalize, tr_a.augment.autocontrast, tr_a.augment.autocontrast_cutoff) == (0.4, 0.6, 5.0)
    assert _epoch_line(out_a) == _epoch_line(out_b)
    assert torch.isfinite(tr_a.net.flat_params).all() and torch.equal(tr_a.net.flat_params, tr_b.net.flat_params)


@pytest.mark.parametrize("extra", [["--keep_aspect"], ["--train_tiles", "2x2", "--tile_overlap", "32"], ["--aug_jpeg", "40", "--aug_blur", "2"]],
                         ids=["keep_aspect", "train_tiles", "jpeg_blur"])
def test_train_cli_with_the_flags_beside_the_other_flags(golden_dir, tmp_path, monkeypatch, capsys, extra):
    from tests.helpers import write_evaluate16_dir
    from tests.test_gpu_blur import _epoch_line
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr, out = _train_run(tmp_path, "run", extra, monkeypatch, capsys)
    _epoch_line(out)
    assert tr.augment.equalize == 0.4 and torch.isfinite(tr.net.flat_params).all()


def test_train_cli_refuses_the_flags_with_synthetic(tmp_path, monkeypatch):
    from structuredetector_amd.cli import train
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="'aug_equalize' / 'aug_autocontrast' work on source images: they need --train_dir, not --synthetic"):
        train.main(_train_args(tmp_path, ["--synthetic", "8"]))
