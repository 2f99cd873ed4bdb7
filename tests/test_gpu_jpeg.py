"""JPEG compression on the GPU (sd_jpeg_u8: k_jpeg_code, k_jpeg_rgb; sd_preprocess_images_jpeg / _list_jpeg) against tests/jpeg_ref.py --
the numpy restatement that tests/test_jpeg_cpu.py pins to Pillow byte for byte -- bit for bit: the stand-alone stage over sizes around its
64 x 64 tile, arbitrary quantisation tables (the quantiser's division), in place, unaligned views, the refusals, the chain forms against the
hand composition of the existing entry points and jpeg_ref, a null table against the perspective form, `TrainAugmentation` with
`--aug_jpeg` against Pillow's own chain, and `train --aug_jpeg`."""
import functools
import io
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.jpeg_ref import jpeg_quant_tables, jpeg_ref, jpeg_roundtrip

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (height, width): one MCU (every upsample edge at once), one MCU row / column, a few MCUs, and sizes around the kernel's 64 x 64 tile: the
# tile itself, one MCU more on either axis (80 = 64 + 16), one MCU less (48), and several tiles with a partial one on both axes (144 x 176)
SHAPES = [(16, 16), (16, 48), (48, 16), (32, 32), (48, 80), (64, 96), (144, 176), (64, 64), (80, 64), (64, 80)]
QUALITIES = [0, 1, 10, 50, 75, 95, 100, 100, 95, 75, 50, 10, 1, 0]   # a copy row at either end; every quality on two kinds of image
KINDS = ["noise", "saturated", "smooth", "constant"]


def _image(kind, h, w, rng):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "saturated":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if kind == "constant":
        return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()
    if kind == "extreme":                                            # block (i, j) is the sign pattern of the DCT basis (i % 8, j % 8): the largest coefficients
        y, x = np.mgrid[0:h, 0:w]
        basis = np.cos((2 * (y % 8) + 1) * ((y // 8) % 8) * np.pi / 16) * np.cos((2 * (x % 8) + 1) * ((x // 8) % 8) * np.pi / 16)
        return np.repeat(((basis > 0) * 255).astype(np.uint8)[..., None], 3, axis=2)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)                     # smooth: ramps and a slow wave
    chans = [255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 127.5 + 127.5 * np.sin(x / 9.0 + y / 13.0)]
    return np.stack(chans, axis=-1).round().astype(np.uint8)


def _row(quality):
    if quality == 0:
        return [0] + [1] * 128
    ql, qc = jpeg_quant_tables(quality)
    return [1, *ql.reshape(-1).tolist(), *qc.reshape(-1).tolist()]


@functools.lru_cache(maxsize=None)
def _stage_case(shape):
    """Images, table rows and the expected bytes of one shape: computed once, read only."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    imgs = np.stack([_image(KINDS[i % 4], h, w, rng) for i in range(len(QUALITIES))])
    rows = [_row(q) for q in QUALITIES]
    want = np.stack([jpeg_ref(a, q) for a, q in zip(imgs, QUALITIES)])
    imgs.setflags(write=False); want.setflags(write=False)
    return imgs, rows, want


def _differences(got, want, rows, what):
    for b in range(len(rows)):
        bad = got[b] != want[b]
        assert not bad.any(), f"{what} row {b}: {bad.sum()} bytes differ, first at {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_sd_jpeg_u8_matches_the_reference_bitwise(shape):
    from structuredetector_amd.data import jpeg_images
    imgs, rows, want = _stage_case(shape)
    assert (want[1:-1] != imgs[1:-1]).any() and np.array_equal(want[0], imgs[0])
    x = torch.tensor(imgs, device=DEV)
    got = jpeg_images(x, rows).cpu().numpy()
    assert np.array_equal(x.cpu().numpy(), imgs)                     # the input is read only
    _differences(got, want, rows, shape)
    # the same rows in another order: a block reads its own image's row of the table
    perm = list(range(len(rows)))[::-1]
    again = jpeg_images(torch.tensor(imgs[perm], device=DEV), [rows[i] for i in perm]).cpu().numpy()
    assert np.array_equal(again, want[perm])


def test_arbitrary_tables_exercise_the_quantiser():
    """Constant tables, random tables and tables with entries outside [1, 255] (clamped on the device), on noise, saturated and
    largest-coefficient images: the quantiser's reciprocal divides exactly for every 8 q."""
    from structuredetector_amd.data import jpeg_images
    h, w = 64, 64
    rng = np.random.default_rng(12)
    tables = [(np.full(64, v), np.full(64, v)) for v in (1, 2, 3, 5, 7, 13, 64, 127, 251, 255)]
    tables += [(rng.integers(1, 256, 64), rng.integers(1, 256, 64)) for _ in range(6)]
    tables.append((np.arange(1, 65), np.arange(255, 191, -1)))
    imgs, rows, want = [], [], []
    for k, (ql, qc) in enumerate(tables):
        for kind in ("noise", "saturated", "extreme"):
            a = _image(kind, h, w, rng)
            imgs.append(a); rows.append([1 + k, *ql.tolist(), *qc.tolist()])           # any non-zero `on` compresses
            want.append(jpeg_roundtrip(a, ql, qc))
    wild = rng.integers(1, 256, 128)
    for bad in (0, -4, 300, 2 ** 31 - 1):
        t = wild.copy()
        t[rng.integers(0, 128, 24)] = bad
        t[0] = t[64] = bad                                           # the DC entries too
        a = _image("noise", h, w, rng)
        imgs.append(a); rows.append([1, *t.tolist()])
        c = np.clip(t, 1, 255)
        want.append(jpeg_roundtrip(a, c[:64], c[64:]))
    got = jpeg_images(torch.tensor(np.stack(imgs), device=DEV), rows).cpu().numpy()
    _differences(got, np.stack(want), rows, "tables")


def _raw_call(src_ptr, dst_ptr, B, H, W, table, ws=None, ws_bytes=None):
    from structuredetector_amd import _lib as L
    lib = L.lib()
    if ws is None:
        ws = L.workspace(lib.sd_jpeg_workspace_bytes(B, H, W), torch.device(DEV, torch.cuda.current_device()))
    table_ptr = table.data_ptr() if table is not None else 0
    return lib.sd_jpeg_u8(src_ptr, dst_ptr, B, H, W, table_ptr, ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, L.stream()), lib


def test_in_place_gives_the_same_bytes():
    imgs, rows, want = _stage_case((144, 176))
    x = torch.tensor(imgs, device=DEV)
    table = torch.tensor(np.asarray(rows, dtype=np.int32), device=DEV)
    code, _ = _raw_call(x.data_ptr(), x.data_ptr(), *imgs.shape[:3], table)
    assert code == 0
    assert np.array_equal(x.cpu().numpy(), want)


def test_sd_jpeg_u8_on_views_that_are_not_16_byte_aligned():
    """A base address that is not 16-byte aligned: the byte path gives the same bytes, and nothing outside the images is written."""
    imgs, rows, want = _stage_case((64, 96))
    B, H, W = imgs.shape[:3]
    n = imgs.size
    arena_in = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
    arena_in[5:5 + n].copy_(torch.tensor(imgs, device=DEV).reshape(-1))
    table = torch.tensor(np.asarray(rows, dtype=np.int32), device=DEV)
    for a, o in ((5, 3), (4, 8)):                                    # odd addresses; dword-aligned ones that are not 16-byte aligned
        arena_out = torch.full((n + 64,), 7, dtype=torch.uint8, device=DEV)
        src = arena_in[5:5 + n] if a == 5 else arena_in[5:5 + n].clone()
        if a != 5:
            shifted = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
            shifted[a:a + n].copy_(src)
            src = shifted[a:a + n]
        assert src.data_ptr() % 16 == a
        code, _ = _raw_call(src.data_ptr(), arena_out.data_ptr() + o, B, H, W, table)
        assert code == 0
        out = arena_out.cpu().numpy()
        assert np.array_equal(out[o:o + n].reshape(imgs.shape), want), (a, o)
        assert (out[:o] == 7).all() and (out[o + n:] == 7).all()     # nothing outside the images is written
    code, _ = _raw_call(arena_in.data_ptr() + 5, arena_in.data_ptr() + 5, B, H, W, table)     # in place, unaligned
    assert code == 0
    assert np.array_equal(arena_in.cpu().numpy()[5:5 + n].reshape(imgs.shape), want)
    assert not arena_in[:5].any() and not arena_in[5 + n:].any()


def test_bad_calls_are_refused_before_any_launch():
    from structuredetector_amd import _lib as L
    H, W = 48, 80
    x = torch.full((2, H, W, 3), 9, dtype=torch.uint8, device=DEV)
    out = torch.full((2, H, W, 3), 3, dtype=torch.uint8, device=DEV)
    table = torch.tensor(np.asarray([_row(50), _row(10)], dtype=np.int32), device=DEV)
    dev = torch.device(DEV, torch.cuda.current_device())
    full = L.lib().sd_jpeg_workspace_bytes(2, H, W)
    assert full == 2 * H * W * 3 // 2
    invalid, too_small = -1, -2                                      # SD_ERR_INVALID, SD_ERR_WORKSPACE
    cases = [(dict(H=24), invalid, "MCU"), (dict(W=40), invalid, "MCU"), (dict(table=None), invalid, "null"),
             (dict(ws_bytes=full - 1), too_small, f"workspace {full - 1} < {full}"), (dict(dst=x.data_ptr() + 3 * W), invalid, "overlap")]
    for kw, expected, text in cases:
        code, lib = _raw_call(x.data_ptr(), kw.get("dst", out.data_ptr()), 2, kw.get("H", H), kw.get("W", W), kw.get("table", table),
                              L.workspace(full, dev), kw.get("ws_bytes"))
        assert code == expected, (kw, code)
        msg = lib.sd_last_error().decode()
        assert "sd_jpeg_u8" in msg and text in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (out == 3).all() and (x == 9).all()                       # no launch was left behind
    from structuredetector_amd.data import jpeg_images
    with pytest.raises(L.SdError, match="MCU"):
        jpeg_images(torch.zeros((1, 24, 32, 3), dtype=torch.uint8, device=DEV), [_row(50)])
    with pytest.raises(L.SdError, match="one row"):
        jpeg_images(x, [_row(50)])


# ---- the chain forms -------------------------------------------------------------------------------------------------------------
CHAIN_Q = [0, 10, 50, 90]                                            # one image of the batch stays as it is


def _persp(size, n):
    from structuredetector_amd.data import compose_affine_perspective, perspective_coeffs
    from tests.test_gpu_train_tiles import _warps
    W, H = size
    frame = [(0.0, 0.0), (float(W), 0.0), (float(W), float(H)), (0.0, float(H))]
    quads = [[(1.5 + b, 2.0), (W - 3.0, 0.5 * b), (W - 1.0 - b, H - 2.5), (2.0 * b, H - 1.0)] for b in range(n)]
    return [compose_affine_perspective(m, perspective_coeffs(frame, q)) for m, q in zip(_warps(size, n), quads)]


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_chain_forms_equal_the_hand_composition(geometry):
    """The existing chain up to the blur (its bytes read back from the existing entry point), jpeg_ref on the host, then the existing
    jitter / flips / normalise on those bytes (an identity resize): the packed and the list form give that tensor bit for bit, for the
    stage sets of the blur's test, each with and without the blur and with the warp as an affine matrix or folded into a homography."""
    from structuredetector_amd.data import blur_box_params, preprocess_image_list, preprocess_images
    from tests.test_gpu_blur import NB, OUT, RADII, SRC, _bytes, _geometry, _sources, _stage_sets, _table
    x = torch.tensor(_sources(), device=DEV)
    arena, table = _table()
    geom = _geometry(geometry)
    rows = [_row(q) for q in CHAIN_Q]
    blur = [blur_box_params(r) for r in RADII]
    for name, front, behind in _stage_sets():
        for with_blur in (False, True):
            for with_persp in (False, True):
                head_kw = dict(front)
                if with_persp:                                       # the warp slot holds one homography: the affine draw is folded in
                    head_kw.pop("affine", None)
                    head_kw["persp"] = _persp(OUT, NB)
                if with_blur:
                    head_kw["blur"] = blur
                tag = f"{geometry} {name} blur={with_blur} persp={with_persp}"
                head = preprocess_images(x, OUT, **geom, **head_kw)
                u8 = _bytes(head)
                assert torch.equal(preprocess_images(torch.tensor(u8, device=DEV), OUT), head), tag     # the bytes, and the identity resize
                coded = np.stack([jpeg_ref(u8[b], CHAIN_Q[b]) for b in range(NB)])
                assert np.array_equal(coded[0], u8[0]) and all((coded[b] != u8[b]).any() for b in range(1, NB))
                want = preprocess_images(torch.tensor(coded, device=DEV), OUT, **behind)
                for form, got in (("packed", preprocess_images(x, OUT, **geom, **head_kw, **behind, jpeg=rows)),
                                  ("list", preprocess_image_list(table, SRC[0], SRC[1], OUT, **geom, **head_kw, **behind, jpeg=rows))):
                    if "jitter" not in behind:                       # the bytes themselves
                        bad = (_bytes(got) != _bytes(want)).sum()
                        assert bad == 0, f"{form} {tag}: {bad} bytes differ"
                    assert torch.equal(got, want), f"{form} {tag}: {(got != want).sum().item()} values differ"
    del arena


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_a_null_table_is_the_perspective_form_bit_for_bit(geometry):
    from structuredetector_amd.data import blur_box_params, preprocess_image_list, preprocess_images
    from structuredetector_amd.data.augment import _MEAN, _STD
    from tests.helpers import call_legacy_preprocess_form as _preprocess_blur
    from tests.test_gpu_blur import NB, OUT, RADII, SRC, _geometry, _sources, _stage_sets, _table
    x = torch.tensor(_sources(), device=DEV)
    arena, table = _table()
    geom = _geometry(geometry)
    for name, front, behind in _stage_sets():
        for extra in ({}, dict(blur=[blur_box_params(r) for r in RADII]), dict(persp=_persp(OUT, NB))):
            kw = dict(flips=None, jitter=None, affine=None, mosaic=None, window=None, letterbox=None, blur=None, persp=None)
            kw.update(geom); kw.update(front); kw.update(behind); kw.update(extra)
            if kw["persp"] is not None:
                kw["affine"] = None
            stages = {k: v for k, v in kw.items() if v is not None}
            args = (NB, SRC[0], SRC[1], OUT, kw["flips"], _MEAN, _STD, kw["jitter"], kw["affine"], kw["mosaic"], kw["window"], kw["letterbox"], kw["blur"],
                    x.device, kw["persp"], None)
            want = preprocess_images(x, OUT, **stages)
            assert torch.equal(_preprocess_blur("sd_preprocess_images_jpeg", x.data_ptr(), *args), want), (name, sorted(extra))
            want = preprocess_image_list(table, SRC[0], SRC[1], OUT, **stages)
            assert torch.equal(_preprocess_blur("sd_preprocess_images_list_jpeg", table.data_ptr(), *args), want), (name, sorted(extra))
    del arena


def test_chain_rejects_what_it_cannot_do():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import preprocess_images
    x = torch.zeros((1, 20, 20, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.SdError, match="16 x 16 MCUs"):
        preprocess_images(x, (24, 16), jpeg=[_row(50)])
    with pytest.raises(L.SdError, match="one row"):
        preprocess_images(x, (16, 16), jpeg=[_row(50)] * 2)
    with pytest.raises(L.SdError, match="do not combine"):
        preprocess_images(x, (16, 16), jpeg=[_row(50)], persp=[[1.0, 0, 0, 0, 1.0, 0, 0, 0]], affine=[[1.0, 0, 0, 0, 1.0, 0]])


# ---- the augmentation class and the CLI ------------------------------------------------------------------------------------------
def _pillow_chain(img, size, quality, jit, hflip, vflip):
    """Resize -> save(JPEG, quality) + open -> ColorJitter -> flips -> to_tensor -> Normalize, every image operation Pillow's own."""
    from PIL import Image
    from tests.test_gpu_pipeline import MEAN, STD, pil_color_jitter
    im = Image.fromarray(img).resize(size, Image.BILINEAR)
    if quality > 0:
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=quality)
        buf.seek(0)
        im = Image.open(buf).convert("RGB")
    im = pil_color_jitter(im, *jit)
    if hflip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if vflip:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    return torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).to(torch.float32).div(255).sub(MEAN).div(STD)


def test_train_augmentation_with_aug_jpeg_equals_the_pillow_chain():
    from structuredetector_amd.data import TrainAugmentation
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    size, n = (96, 64), 6
    rng = np.random.default_rng(9)
    imgs = [_image("smooth", 60, 80, rng) // 2 + rng.integers(0, 128, (60, 80, 3), dtype=np.uint8) for _ in range(n)]
    make_anns = lambda: [ImageAnnotation(f"{i}.png", [Object("bean", Keypoint("stem", 10.0 * i + 1, 5.0 * i + 2), [])]) for i in range(n)]
    common = dict(width=size[0], height=size[1], no_augmentation=False, device=torch.device(DEV))
    outs = {}
    for qmin in (30, 0):
        aug = TrainAugmentation(Namespace(**common, aug_jpeg=qmin))
        torch.manual_seed(21)
        flips, (words, factors) = aug.draws_for(n)                   # the draws the call below makes, in its order
        qualities = aug.jpeg_draws_for(n)
        torch.manual_seed(21)
        out, anns = aug(imgs, make_anns())
        if qmin:
            assert any(q > 0 for q in qualities) and any(q == 0 for q in qualities) and all(q == 0 or 30 <= q <= 95 for q in qualities)
        else:
            assert qualities is None
        for i in range(n):
            order = [(words[i] >> (2 * k)) & 3 for k in range(4)]
            jit = (order, *factors[i], ((words[i] >> 8) & 255,))
            want = _pillow_chain(imgs[i], size, qualities[i] if qualities else 0, jit, bool(flips[i] & 1), bool(flips[i] & 2))
            assert torch.equal(out[i].cpu(), want), f"aug_jpeg {qmin} image {i}: {(out[i].cpu() != want).sum().item()} values differ"
        outs[qmin] = (out.cpu(), [(a.objects[0].x, a.objects[0].y) for a in anns])
    assert outs[30][1] == outs[0][1]                                 # photometric: the annotations are those of the plain chain
    assert not torch.equal(outs[30][0], outs[0][0])


def _train_args(tmp_path, source):
    return source + ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "-b", "4", "-e", "1", "--steps", "2",
                     "--decode_workers", "2", "--aug_jpeg", "30"]


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


def test_train_cli_with_aug_jpeg_with_and_without_the_image_cache(golden_dir, tmp_path, monkeypatch, capsys):
    """Two steps of `train --aug_jpeg 30` from a PNG + JSON directory: finite losses, identical with and without --cache_images (the packed
    and the pointer-list form of the chain)."""
    from tests.helpers import write_evaluate16_dir
    from tests.test_gpu_blur import _epoch_line
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr_a, out_a = _train_run(tmp_path, "plain", [], monkeypatch, capsys)
    tr_b, out_b = _train_run(tmp_path, "cached", ["--cache_images", "0.5"], monkeypatch, capsys)
    assert tr_a.cache is None and tr_b.cache is not None and tr_a.augment.jpeg == 30
    assert _epoch_line(out_a) == _epoch_line(out_b)
    assert torch.isfinite(tr_a.net.flat_params).all() and torch.equal(tr_a.net.flat_params, tr_b.net.flat_params)


@pytest.mark.parametrize("extra", [["--keep_aspect"], ["--train_tiles", "2x2", "--tile_overlap", "32"],
                                   ["--aug_blur", "2", "--aug_perspective", "0.3", "--aug_rotate", "10", "--aug_mosaic", "0.5"]],
                         ids=["keep_aspect", "train_tiles", "every_stage"])
def test_train_cli_with_aug_jpeg_beside_the_other_flags(golden_dir, tmp_path, monkeypatch, capsys, extra):
    from tests.helpers import write_evaluate16_dir
    from tests.test_gpu_blur import _epoch_line
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    tr, out = _train_run(tmp_path, "run", extra, monkeypatch, capsys)
    _epoch_line(out)
    assert tr.augment.jpeg == 30 and torch.isfinite(tr.net.flat_params).all()


def test_train_cli_refuses_aug_jpeg_with_synthetic(tmp_path, monkeypatch):
    from structuredetector_amd.cli import train
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="'aug_jpeg' compresses source images: it needs --train_dir, not --synthetic"):
        train.main(_train_args(tmp_path, ["--synthetic", "8"]))
