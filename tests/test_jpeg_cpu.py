"""JPEG compression augmentation (`--aug_jpeg`), the parts that need no GPU: tests/jpeg_ref.py against Pillow's own save / open round trip
byte for byte, the quantisation tables against `Image.open().quantization`, the host helpers of data/augment.py against the reference's,
the flag and its refusals, the extra training draw, and the argument validation of `sd_jpeg_u8` (host code that runs before any launch)."""
import io
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.jpeg_ref import jpeg_quant_tables, jpeg_ref, jpeg_roundtrip


def _pillow(a, **kw):
    """(H, W, 3) uint8 -> (the decoded image, the file's quantisation tables) of Pillow's save(JPEG, **kw) then open()."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    buf.seek(0)
    im = Image.open(buf)
    return np.asarray(im.convert("RGB")), im.quantization


def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _saturated(rng, h, w):
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def _smooth(rng, h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    p = rng.uniform(0, 6, 3)
    return np.stack([127.5 + 127.5 * np.sin(x / 7.0 + y / 11.0 + p[0]), 255 * x / max(w - 1, 1), 127.5 + 127.5 * np.cos(y / 5.0 + p[2])], -1).round().astype(np.uint8)


def test_jpeg_ref_is_pillow_byte_for_byte_at_every_quality():
    """Every quality from 1 to 100 on 32 x 32, noise and saturated images alternating: zero differing bytes, and the same tables."""
    rng = np.random.default_rng(0)
    for q in range(1, 101):
        a = _noise(rng, 32, 32) if q % 2 else _saturated(rng, 32, 32)
        want, tables = _pillow(a, quality=q)
        ql, qc = jpeg_quant_tables(q)
        assert ql.reshape(-1).tolist() == list(tables[0]) and qc.reshape(-1).tolist() == list(tables[1]), q
        got = jpeg_ref(a, q)
        assert np.array_equal(got, want), f"quality {q}: {(got != want).sum()} bytes differ"


@pytest.mark.parametrize("shape", [(16, 16), (16, 48), (48, 16), (64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_jpeg_ref_is_pillow_byte_for_byte_over_sizes_and_images(shape):
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    for q in (10, 30, 50, 75, 95):
        for make in (_noise, _saturated, _smooth):
            a = make(rng, *shape)
            want, _ = _pillow(a, quality=q)
            got = jpeg_ref(a, q)
            assert np.array_equal(got, want), f"{shape} quality {q} {make.__name__}: {(got != want).sum()} bytes differ"


def test_jpeg_ref_is_pillow_byte_for_byte_with_arbitrary_tables():
    rng = np.random.default_rng(5)
    cases = [(rng.integers(1, 256, 64), rng.integers(1, 256, 64)) for _ in range(12)]
    cases += [(np.full(64, v), np.full(64, v)) for v in (1, 2, 3, 5, 7, 13, 64, 127, 251, 255)]
    for k, (ql, qc) in enumerate(cases):
        a = (_noise, _saturated, _smooth)[k % 3](rng, 48, 64)
        want, tables = _pillow(a, qtables=[ql.tolist(), qc.tolist()], subsampling=2)
        assert list(tables[0]) == ql.tolist() and list(tables[1]) == qc.tolist()          # natural order in, natural order out
        got = jpeg_roundtrip(a, ql, qc)
        assert np.array_equal(got, want), f"table {k}: {(got != want).sum()} bytes differ"


def test_quant_tables_are_the_values_the_issue_pins():
    from tests.jpeg_ref import BASE_CHROMA, BASE_LUMA
    ql, qc = jpeg_quant_tables(50)
    assert np.array_equal(ql, BASE_LUMA) and np.array_equal(qc, BASE_CHROMA)
    assert ql[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and ql[1].tolist() == [12, 12, 14, 19, 26, 58, 60, 55]
    assert qc[0].tolist() == [17, 18, 24, 47, 99, 99, 99, 99] and qc[1].tolist() == [18, 21, 26, 66, 99, 99, 99, 99]
    assert jpeg_quant_tables(10)[0][0].tolist() == [80, 55, 50, 80, 120, 200, 255, 255]
    assert all((t == 1).all() for t in jpeg_quant_tables(100))


def test_host_helpers_equal_the_reference():
    from structuredetector_amd.data import jpeg_quant_tables as host_tables, jpeg_rows
    for q in range(1, 101):
        hl, hc = host_tables(q)
        rl, rc = jpeg_quant_tables(q)
        assert hl == rl.reshape(-1).tolist() and hc == rc.reshape(-1).tolist(), q
        assert all(type(v) is int for v in hl + hc)
    for bad in (0, -1, 101):
        with pytest.raises(ValueError, match="jpeg quality"):
            host_tables(bad)
    rows = jpeg_rows([0, 10, 95])
    assert [len(r) for r in rows] == [129] * 3
    assert rows[0][0] == 0 and all(1 <= v <= 255 for v in rows[0][1:])                  # the copy row
    for row, q in zip(rows[1:], (10, 95)):
        hl, hc = host_tables(q)
        assert row[0] != 0 and row[1:65] == hl and row[65:] == hc


def test_flag_parses_defaults_to_off_and_is_range_checked():
    from structuredetector_amd.utils.args import Arguments, check_aug_jpeg
    parser = Arguments().parser
    assert parser.parse_args([]).aug_jpeg == 0
    assert parser.parse_args(["--aug_jpeg", "30"]).aug_jpeg == 30
    text = " ".join(parser.format_help().split())
    assert "--aug_jpeg QMIN" in text and "save(quality=q)" in text and "not --synthetic" in text
    for bad in ("-5", "4", "96", "100"):
        with pytest.raises(AssertionError, match="aug_jpeg"):
            Arguments().parse(["--aug_jpeg", bad])
    with pytest.raises(SystemExit):                                                     # an integer flag
        parser.parse_args(["--aug_jpeg", "30.5"])
    assert check_aug_jpeg(parser.parse_args(["--aug_jpeg", "5"])) == 5
    assert check_aug_jpeg(parser.parse_args([])) == 0
    assert check_aug_jpeg(Namespace()) == 0                                             # a namespace from before the flag
    assert check_aug_jpeg(parser.parse_args(["--aug_jpeg", "95"])) == 95
    assert check_aug_jpeg(parser.parse_args(["--synthetic", "8"])) == 0                 # off: --synthetic is fine
    for bad in (-1, 4, 96, 30.5, float("nan")):
        with pytest.raises(ValueError, match="aug_jpeg"):
            check_aug_jpeg(Namespace(aug_jpeg=bad))
    with pytest.raises(ValueError, match="'aug_jpeg' compresses source images: it needs --train_dir, not --synthetic"):
        check_aug_jpeg(parser.parse_args(["--aug_jpeg", "30", "--synthetic", "8"]))
    from structuredetector_amd.model.trainer import Trainer
    with pytest.raises(ValueError, match="needs --train_dir, not --synthetic"):         # `train` checks before it builds anything (no GPU is touched)
        Trainer(parser.parse_args(["--aug_jpeg", "30", "--synthetic", "8"]))


_COMMON = dict(width=128, height=96, no_augmentation=False, aug_rotate=10.0, aug_mosaic=0.5, aug_transpose=0.0, train_tiles="", device="cpu")


def test_no_draw_when_off_and_one_draw_when_on():
    from structuredetector_amd.data import TrainAugmentation, ValidationAugmentation
    for extra in (dict(), dict(aug_jpeg=0), dict(aug_jpeg=30, no_augmentation=True)):
        aug = TrainAugmentation(Namespace(**{**_COMMON, **extra}))
        torch.manual_seed(3)
        before = torch.get_rng_state()
        assert aug.jpeg_draws_for(6) is None
        assert torch.equal(torch.get_rng_state(), before), extra                        # no draw at all
    val = ValidationAugmentation(Namespace(width=128, height=96, aug_jpeg=30))
    before = torch.get_rng_state()
    assert val.jpeg_draws_for(6) is None and torch.equal(torch.get_rng_state(), before)
    for qmin in (5, 30, 95):
        aug = TrainAugmentation(Namespace(**_COMMON, aug_jpeg=qmin))
        torch.manual_seed(3)
        qualities = aug.jpeg_draws_for(256)
        torch.manual_seed(3)
        u = torch.rand(256, 2, dtype=torch.float64).tolist()                            # ONE draw: rand(n, 2) in float64
        after = torch.get_rng_state()
        assert qualities == [min(95, qmin + int(u1 * (96 - qmin))) if u0 < 0.5 else 0 for u0, u1 in u]
        torch.manual_seed(3)
        aug.jpeg_draws_for(256)
        assert torch.equal(torch.get_rng_state(), after)
        assert any(q == 0 for q in qualities) and all(q == 0 or qmin <= q <= 95 for q in qualities)
        assert qmin == 95 or len({q for q in qualities if q}) > 1


def test_the_draw_comes_after_the_perspective_draw_and_changes_no_earlier_one():
    """Flips, jitter, warp, mosaic, window, transpose, blur and perspective draws are the same with the flag on and off; with it on, the
    next numbers of the generator are the JPEG draw's."""
    from structuredetector_amd.data import TrainAugmentation
    common = {**_COMMON, "width": 128, "height": 128, "aug_transpose": 0.5, "train_tiles": "2x2", "tile_overlap": 32, "aug_blur": 2.0,
              "aug_perspective": 0.3}
    seen = []
    n, groups = 8, [[0, 1, 2, 3], [4, 5, 6, 7]]
    for qmin in (0, 30):
        aug = TrainAugmentation(Namespace(**common, aug_jpeg=qmin))
        torch.manual_seed(11)
        seen.append((aug.draws_for(n), aug.affine_draws_for(n), aug.mosaic_draws_for(n, groups), aug.window_draws_for(n), aug.transpose_draws_for(n),
                     aug.blur_draws_for(n), aug.perspective_draws_for(n)))
        state = torch.get_rng_state()
        tail = aug.jpeg_draws_for(n)
        assert (tail is None) == (qmin == 0)
        if qmin:
            torch.set_rng_state(state)
            u = torch.rand(n, 2, dtype=torch.float64).tolist()
            assert tail == [min(95, 30 + int(u1 * 66)) if u0 < 0.5 else 0 for u0, u1 in u]
    assert seen[0] == seen[1]


def test_library_exports_the_jpeg_symbols():
    from structuredetector_amd import _lib as L
    handle = L.lib()
    names = {"sd_jpeg_u8", "sd_jpeg_workspace_bytes", "sd_preprocess_images_jpeg", "sd_preprocess_images_list_jpeg",
             "sd_preprocess_jpeg_workspace_bytes"}
    assert names <= set(L.declared_symbols())
    assert all(hasattr(handle, n) for n in names)
    assert handle.sd_jpeg_workspace_bytes(2, 16, 16) == 768                             # 1.5 bytes per pixel
    assert handle.sd_jpeg_workspace_bytes(1, 16, 16) == 512                             # 384 bytes, rounded up to 256
    for geometry, g in ((0, (0, 0)), (1, (0, 30)), (2, (32, 0))):                       # the blur form's size plus the planes
        args = (geometry, 4, 40, 56, g[0], 32, 32, g[1])
        assert handle.sd_preprocess_jpeg_workspace_bytes(*args) == handle.sd_preprocess_blur_workspace_bytes(*args) + 4 * 32 * 32 * 3 // 2


def test_sd_jpeg_u8_rejects_bad_arguments_without_touching_the_gpu():
    """Every bad call returns before a launch (the pointers are never dereferenced) and sd_last_error() names the function."""
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def call(src=16, dst=1 << 20, B=2, H=32, W=48, table=2 << 20, ws=3 << 20, ws_bytes=4608):
        return lib.sd_jpeg_u8(src, dst, B, H, W, table, ws, ws_bytes, 0)

    for kw, code, text in [(dict(src=0), -1, "null"), (dict(dst=0), -1, "null"), (dict(table=0), -1, "null"), (dict(ws=0), -1, "null"),
                           (dict(B=0), -1, "bad shape"), (dict(H=0), -1, "bad shape"), (dict(W=-16), -1, "bad shape"), (dict(H=24), -1, "MCU"),
                           (dict(W=40), -1, "MCU"), (dict(H=8, W=8), -1, "MCU"), (dict(B=70000), -1, "too large"), (dict(dst=16 + 48), -1, "overlap"),
                           (dict(ws=(3 << 20) + 4), -1, "aligned"), (dict(ws_bytes=4607), -2, "workspace 4607 < 4608")]:
        assert call(**kw) == code, kw
        msg = lib.sd_last_error().decode()
        assert "sd_jpeg_u8" in msg and text in msg, (kw, msg)
