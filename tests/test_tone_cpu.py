"""The host half of `--aug_equalize` / `--aug_autocontrast` without a GPU: tests/tone_ref.py (the closed forms the kernels restate) against
Pillow's ImageOps.equalize and ImageOps.autocontrast byte for byte, the double-precision stretch table against Python's own floats over
every (lo, hi) pair, the table rows, the flags and their checks, the draw discipline, and the C ABI's declarations and refusals."""
import re
from argparse import Namespace
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.tone_ref import (AUTOCONTRAST, COPY, EQUALIZE, KINDS, autocontrast_lo_hi, cut_of, equalize_lut, pillow_tone, stretch_lut,
                            tone_image, tone_ref)

SIZES = [(1, 1), (1, 5), (2, 2), (3, 7), (15, 17), (16, 16), (37, 53), (60, 59)]
CUTOFFS = [0, 0.001, 0.5, 1.0, 2.5, 10, 25.0, 39.9, 40]


def test_equalize_equals_pillow():
    rng = np.random.default_rng(1)
    changed = 0
    for h, w in SIZES:
        for kind in KINDS:
            for _ in range(3):
                img = tone_image(kind, h, w, rng)
                want = pillow_tone(img, EQUALIZE)
                got = tone_ref(img, [EQUALIZE, 0, 0, 0])
                assert np.array_equal(got, want), (h, w, kind)
                changed += int((want != img).any())
    assert changed > 20


def test_autocontrast_equals_pillow():
    rng = np.random.default_rng(2)
    changed = 0
    for h, w in SIZES:
        for kind in KINDS:
            img = tone_image(kind, h, w, rng)
            for cutoff in CUTOFFS:
                want = pillow_tone(img, AUTOCONTRAST, cutoff)
                cut = cut_of(h * w, cutoff)
                got = tone_ref(img, [AUTOCONTRAST, cut, cut, 0])
                assert np.array_equal(got, want), (h, w, kind, cutoff)
                changed += int((want != img).any())
    assert changed > 50


def test_copy_modes_and_clamped_cuts():
    rng = np.random.default_rng(3)
    img = tone_image("narrow", 9, 11, rng)
    for mode in (COPY, 7, -1):
        assert np.array_equal(tone_ref(img, [mode, 3, 3, 0]), img)
    assert np.array_equal(tone_ref(img, [AUTOCONTRAST, -5, -5, 0]), pillow_tone(img, AUTOCONTRAST, 0))          # clamped to 0
    assert np.array_equal(tone_ref(img, [AUTOCONTRAST, 2 ** 31 - 1, 0, 0]), img)                                # clamped to n: every pixel is cut


def test_a_cut_that_empties_a_bin_exactly():
    """cut == h[lo]: Pillow's loop empties the bin and stops; lo is the NEXT non-empty bin."""
    img = np.empty((10, 10, 3), dtype=np.uint8)
    flat = np.concatenate([np.full(5, 10), np.full(60, 50), np.full(30, 120), np.full(5, 200)]).astype(np.uint8)
    img[...] = flat.reshape(10, 10, 1)
    h = np.bincount(flat, minlength=256)
    assert cut_of(100, 5.0) == 5 == h[10] == h[200]
    assert autocontrast_lo_hi(h, 5, 5) == (50, 120)
    assert autocontrast_lo_hi(h, 4, 4) == (10, 200)
    for cutoff in (5.0, 4.0, 6.0):
        cut = cut_of(100, cutoff)
        assert np.array_equal(tone_ref(img, [AUTOCONTRAST, cut, cut, 0]), pillow_tone(img, AUTOCONTRAST, cutoff)), cutoff


def test_equalize_with_fewer_than_255_pixels_is_the_identity():
    rng = np.random.default_rng(4)
    img = tone_image("noise", 9, 28, rng)                            # n = 252: step == 0
    assert (252 - 1) // 255 == 0
    assert np.array_equal(pillow_tone(img, EQUALIZE), img) and np.array_equal(tone_ref(img, [EQUALIZE, 0, 0, 0]), img)


def test_equalize_saturates_where_the_quotient_exceeds_255():
    """n - last = 300 and step = 1: the entry of the highest bin is 300, which Pillow's point() saturates to 255."""
    flat = np.concatenate([np.arange(300) % 150, np.full(100, 240)]).astype(np.uint8)
    img = np.repeat(flat.reshape(20, 20, 1), 3, axis=2)
    h = np.bincount(flat, minlength=256).astype(np.int64)
    step = (400 - 100) // 255
    below = np.concatenate([[0], np.cumsum(h)[:-1]])
    assert step == 1 and (step // 2 + below[240]) // step == 300 and ((step // 2 + below[:150]) // step > 255).any()
    want = pillow_tone(img, EQUALIZE)
    assert (want[img == 240] == 255).all()
    assert np.array_equal(tone_ref(img, [EQUALIZE, 0, 0, 0]), want)
    assert equalize_lut(h)[240] == 255


def test_the_stretch_table_equals_python_floats_for_every_pair():
    """All 32,640 (lo, hi) pairs: the numpy table equals Python's int(ix * scale + offset), clamped -- Pillow's loop verbatim.  The exact
    integer quotient differs from it in some entries, which is why the kernel must round the product and the sum separately."""
    differ_from_integer = 0
    ix = np.arange(256)
    for lo in range(255):
        for hi in range(lo + 1, 256):
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            want = [min(max(int(i * scale + offset), 0), 255) for i in range(256)]
            got = stretch_lut(lo, hi)
            assert got.tolist() == want, (lo, hi)
            inside = slice(lo, hi + 1)
            differ_from_integer += int((got[inside] != ((ix[inside] - lo) * 255) // (hi - lo)).sum())
    assert differ_from_integer > 0


def test_tone_rows():
    from structuredetector_amd.data import tone_rows
    from structuredetector_amd.data.augment import TONE_AUTOCONTRAST, TONE_COPY, TONE_EQUALIZE
    assert (TONE_COPY, TONE_AUTOCONTRAST, TONE_EQUALIZE) == (COPY, AUTOCONTRAST, EQUALIZE)
    n = 512 * 512
    rows = tone_rows([(EQUALIZE, 0.0), (COPY, 0.0), (AUTOCONTRAST, 1.0), (AUTOCONTRAST, 0.37), (AUTOCONTRAST, 0.0), (EQUALIZE, 3.0)], n)
    assert rows == [[2, 0, 0, 0], [0, 0, 0, 0], [1, 2621, 2621, 0], [1, int(n * 0.37 // 100), int(n * 0.37 // 100), 0], [1, 0, 0, 0], [2, 0, 0, 0]]
    for pixels, c in ((37 * 53, 39.9), (1, 40.0), (100, 5.0), (96 * 131, 0.001), (3000 * 4000, 12.3456)):
        assert tone_rows([(AUTOCONTRAST, c)], pixels) == [[1, cut_of(pixels, c), cut_of(pixels, c), 0]]


def test_flags_parse_default_to_off_and_are_range_checked():
    from structuredetector_amd.utils.args import Arguments, check_aug_tone
    parser = Arguments().parser
    ns = parser.parse_args([])
    assert (ns.aug_equalize, ns.aug_autocontrast, ns.aug_autocontrast_cutoff) == (0.0, 0.0, 1.0)
    ns = parser.parse_args(["--aug_equalize", "0.25", "--aug_autocontrast", "0.5", "--aug_autocontrast_cutoff", "5"])
    assert (ns.aug_equalize, ns.aug_autocontrast, ns.aug_autocontrast_cutoff) == (0.25, 0.5, 5.0)
    assert check_aug_tone(ns) == (0.25, 0.5, 5.0)
    text = " ".join(parser.format_help().split())
    assert "--aug_equalize P" in text and "--aug_autocontrast P" in text and "--aug_autocontrast_cutoff C" in text
    assert "ImageOps.equalize" in text and "ImageOps.autocontrast" in text and "not --synthetic" in text
    for flag, bad in (("--aug_equalize", "-0.1"), ("--aug_equalize", "1.5"), ("--aug_autocontrast", "2"), ("--aug_autocontrast", "-1"),
                      ("--aug_autocontrast_cutoff", "-1"), ("--aug_autocontrast_cutoff", "40.5"), ("--aug_equalize", "nan"),
                      ("--aug_autocontrast_cutoff", "nan")):
        with pytest.raises(AssertionError, match=flag[2:]):
            Arguments().parse([f"{flag}={bad}"])
    assert check_aug_tone(parser.parse_args([])) == (0.0, 0.0, 1.0)
    assert check_aug_tone(Namespace()) == (0.0, 0.0, 1.0)                               # a namespace from before the flags
    assert check_aug_tone(parser.parse_args(["--synthetic", "8"])) == (0.0, 0.0, 1.0)   # off: --synthetic is fine
    assert check_aug_tone(Namespace(aug_equalize=1, aug_autocontrast=1, aug_autocontrast_cutoff=40)) == (1.0, 1.0, 40.0)
    for bad in (dict(aug_equalize=-0.5), dict(aug_equalize=1.01), dict(aug_equalize=float("nan")), dict(aug_autocontrast=3),
                dict(aug_autocontrast=float("nan")), dict(aug_autocontrast="0.5"), dict(aug_autocontrast_cutoff=41),
                dict(aug_autocontrast_cutoff=-0.1), dict(aug_autocontrast_cutoff=float("nan")), dict(aug_equalize=True)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            check_aug_tone(Namespace(**bad))
    for on in (["--aug_equalize", "0.5"], ["--aug_autocontrast", "0.5"]):
        with pytest.raises(ValueError, match="need --train_dir, not --synthetic"):
            check_aug_tone(parser.parse_args(on + ["--synthetic", "8"]))
        from structuredetector_amd.model.trainer import Trainer
        with pytest.raises(ValueError, match="need --train_dir, not --synthetic"):      # `train` checks before it builds anything (no GPU is touched)
            Trainer(parser.parse_args(on + ["--synthetic", "8"]))


_COMMON = dict(width=128, height=128, no_augmentation=False, aug_rotate=10.0, aug_mosaic=0.5, aug_transpose=0.5, train_tiles="2x2", tile_overlap=32,
               aug_blur=2.0, aug_perspective=0.3, aug_jpeg=30, device="cpu")


def _expected(u, p_eq, p_ac, cutoff):
    return [(EQUALIZE, 0.0) if u0 < p_eq else (AUTOCONTRAST, cutoff * u2) if u1 < p_ac else (COPY, 0.0) for u0, u1, u2 in u]


def test_no_draw_when_off_and_one_draw_when_on():
    from structuredetector_amd.data import TrainAugmentation, ValidationAugmentation
    for extra in (dict(), dict(aug_equalize=0.0, aug_autocontrast=0.0), dict(aug_equalize=0.5, aug_autocontrast=0.5, no_augmentation=True),
                  dict(aug_autocontrast_cutoff=5.0)):
        aug = TrainAugmentation(Namespace(**{**_COMMON, **extra}))
        torch.manual_seed(3)
        before = torch.get_rng_state()
        assert aug.tone_draws_for(6) is None
        assert torch.equal(torch.get_rng_state(), before), extra                        # no draw at all
    val = ValidationAugmentation(Namespace(width=128, height=96, aug_equalize=1.0, aug_autocontrast=1.0))
    before = torch.get_rng_state()
    assert val.tone_draws_for(6) is None and torch.equal(torch.get_rng_state(), before)
    for p_eq, p_ac, cutoff in ((0.3, 0.4, 1.0), (1.0, 0.0, 1.0), (0.0, 1.0, 40.0), (0.0, 0.5, 0.0), (1.0, 1.0, 5.0)):
        aug = TrainAugmentation(Namespace(**_COMMON, aug_equalize=p_eq, aug_autocontrast=p_ac, aug_autocontrast_cutoff=cutoff))
        torch.manual_seed(3)
        draws = aug.tone_draws_for(256)
        torch.manual_seed(3)
        u = torch.rand(256, 3, dtype=torch.float64).tolist()                            # ONE draw: rand(n, 3) in float64
        after = torch.get_rng_state()
        assert draws == _expected(u, p_eq, p_ac, cutoff)
        torch.manual_seed(3)
        aug.tone_draws_for(256)
        assert torch.equal(torch.get_rng_state(), after)
        modes = [m for m, _ in draws]
        assert all(m in (COPY, AUTOCONTRAST, EQUALIZE) for m in modes)                  # one outcome per image: never both
        assert all(c == 0.0 for m, c in draws if m != AUTOCONTRAST) and all(0 <= c <= cutoff for _, c in draws)
        if (p_eq, p_ac) == (0.3, 0.4):
            assert {COPY, AUTOCONTRAST, EQUALIZE} == set(modes)
            assert all(m == EQUALIZE for (m, _), (u0, _, _) in zip(draws, u) if u0 < p_eq)        # equalize wins: an image never gets both
        if p_eq == 1.0:
            assert set(modes) == {EQUALIZE}
        if (p_eq, p_ac) == (0.0, 1.0):
            assert set(modes) == {AUTOCONTRAST} and len({c for _, c in draws}) > 100


def test_the_draw_comes_after_the_jpeg_draw_and_changes_no_earlier_one():
    """The draws `__call__` makes, in its order: with the flags off the generator ends where the parent's does; with them on every earlier
    draw is the same and the next numbers of the generator are the tone draw's."""
    from structuredetector_amd.data import TrainAugmentation
    seen, ends = [], []
    n, groups = 8, [[0, 1, 2, 3], [4, 5, 6, 7]]
    for flags in (dict(), dict(aug_equalize=0.0, aug_autocontrast=0.0), dict(aug_equalize=0.3, aug_autocontrast=0.6, aug_autocontrast_cutoff=5.0)):
        aug = TrainAugmentation(Namespace(**_COMMON, **flags))
        torch.manual_seed(11)
        seen.append((aug.draws_for(n), aug.affine_draws_for(n), aug.mosaic_draws_for(n, groups), aug.window_draws_for(n), aug.transpose_draws_for(n),
                     aug.blur_draws_for(n), aug.perspective_draws_for(n), aug.jpeg_draws_for(n)))
        state = torch.get_rng_state()
        tail = aug.tone_draws_for(n)
        ends.append(torch.get_rng_state())
        assert (tail is None) == (not flags.get("aug_equalize"))
        if tail is None:
            assert torch.equal(ends[-1], state)
        else:
            torch.set_rng_state(state)
            u = torch.rand(n, 3, dtype=torch.float64).tolist()
            assert tail == _expected(u, 0.3, 0.6, 5.0) and torch.equal(torch.get_rng_state(), ends[-1])
    assert seen[0] == seen[1] == seen[2] and torch.equal(ends[0], ends[1]) and not torch.equal(ends[0], ends[2])


NAMES = ["sd_tone_workspace_bytes", "sd_tone_u8", "sd_preprocess_tone_workspace_bytes", "sd_preprocess_images_tone", "sd_preprocess_images_list_tone"]


def test_header_declares_and_the_library_exports_the_tone_symbols():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data.augment import TONE_STRIP_PIXELS
    header = (Path(__file__).resolve().parents[1] / "include" / "sdnet_hip.h").read_text()
    for name in NAMES:
        assert re.search(rf"^(size_t|int) {name}\(", header, re.M), name
    assert int(re.search(r"^#define SD_TONE_STRIP_PIXELS (\d+)$", header, re.M).group(1)) == TONE_STRIP_PIXELS
    handle = L.lib()
    assert set(NAMES) <= set(L.declared_symbols())
    assert all(hasattr(handle, n) for n in NAMES)
    assert handle.sd_tone_workspace_bytes(0) == 0 and handle.sd_tone_workspace_bytes(-3) == 0
    assert handle.sd_tone_workspace_bytes(1) == 3072                                    # 3 x 256 uint32 counts
    assert handle.sd_tone_workspace_bytes(3) == 3 * 3072
    for geometry, g in ((0, (0, 0)), (1, (0, 30)), (2, (32, 0))):                       # the JPEG form's size, then the stage's own
        args = (geometry, 4, 40, 56, g[0], 32, 32, g[1])
        assert handle.sd_preprocess_tone_workspace_bytes(*args) == handle.sd_preprocess_jpeg_workspace_bytes(*args) + 4 * 3072
        assert handle.sd_preprocess_tone_workspace_bytes(geometry, 4, 40, 56, g[0], 33, 31, g[1]) > 0                  # no size rule of its own


def test_sd_tone_u8_rejects_bad_arguments_without_touching_the_gpu():
    """Every bad call returns before a launch (the pointers are never dereferenced) and sd_last_error() names the function."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    full = lib.sd_tone_workspace_bytes(2)

    def call(src=16, dst=1 << 20, B=2, H=5, W=7, table=2 << 20, ws=3 << 20, ws_bytes=full):
        return lib.sd_tone_u8(src, dst, B, H, W, table, ws, ws_bytes, 0)

    for kw, code, text in [(dict(src=0), -1, "null"), (dict(dst=0), -1, "null"), (dict(table=0), -1, "null"), (dict(ws=0), -1, "null"),
                           (dict(B=0), -1, "bad shape"), (dict(H=0), -1, "bad shape"), (dict(W=-16), -1, "bad shape"),
                           (dict(B=65536), -1, "65535"), (dict(H=65536, W=32768), -1, "2^31"), (dict(dst=16 + 48), -1, "overlap"),
                           (dict(dst=16 - 1, src=16 + 7), -1, "overlap"), (dict(ws=(3 << 20) + 4), -1, "aligned"),
                           (dict(ws_bytes=full - 1), -2, f"workspace {full - 1} < {full}")]:
        assert call(**kw) == code, kw
        msg = lib.sd_last_error().decode()
        assert "sd_tone_u8" in msg and text in msg, (kw, msg)
