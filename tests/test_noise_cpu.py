"""The host half of `--aug_noise` / `--aug_noise_shot` without a GPU: tests/noise_ref.py (the integer definition the kernel restates) --
Philox4x32-10 against its published known-answer vectors, the unit-normal half table against a fresh statistics.NormalDist computation
and against the array the library owns, the exact integer square root, the statistics of the noise it makes --, the table rows, the flags
and their checks, the draw discipline, and the C ABI's declarations and refusals."""
import ctypes
import importlib.util
import math
import re
from argparse import Namespace
from pathlib import Path
from statistics import NormalDist

import numpy as np
import pytest
import torch

from tests.noise_ref import MAX_A, MAX_B, half_table, isqrt, noise_image, noise_ref, philox4x32_10, rows_of, sigma_table, unit_normals

ROOT = Path(__file__).resolve().parents[1]

KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answer_vectors():
    for counter, key, want in KAT:
        got = tuple(int(w[0]) for w in philox4x32_10(counter, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    # vectorised over counter word 0: element i is the scalar call at counter (i, 0, 0, 0)
    many = philox4x32_10((np.arange(5, dtype=np.uint64), 0, 0, 0), (123, 456))
    for i in range(5):
        assert [int(w[i]) for w in many] == [int(w[0]) for w in philox4x32_10((i, 0, 0, 0), (123, 456))]
    assert [int(w[0]) for w in philox4x32_10((0, 0, 0, 0), (0, 0))] == list(KAT[0][2])


def test_half_table_is_the_fresh_computation_and_the_library_owns_it():
    from structuredetector_amd import _lib as L
    inv = NormalDist().inv_cdf
    fresh = [int(round(1024.0 * inv((2048 + j + 0.5) / 4096.0))) for j in range(2048)]
    h = half_table()
    assert h.tolist() == fresh
    assert h[0] == 0 and h[2047] == 3756 and (np.diff(h) >= 0).all()
    full = np.concatenate([-h[::-1], h]) / 1024.0                    # the 4096 equally likely values of z
    assert abs((full ** 2).mean() - 0.99968) < 5e-5 and abs((full ** 4).mean() / (full ** 2).mean() ** 2 - 2.9915) < 5e-4
    owned = (ctypes.c_uint16 * 2048)()
    assert L.lib().sd_noise_normal_table(ctypes.cast(owned, ctypes.c_void_p)) == 0
    assert list(owned) == fresh
    assert L.lib().sd_noise_normal_table(None) == -1 and "sd_noise_normal_table" in L.lib().sd_last_error().decode()


def test_the_committed_generator_agrees_with_the_source_file():
    spec = importlib.util.spec_from_file_location("noise_table", ROOT / "tools" / "noise_table.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.half_table() == half_table().tolist()
    text = tool.SOURCE.read_text()
    assert text.count(tool.BEGIN) == 1 and text.count(tool.END) == 1
    assert text[text.index(tool.BEGIN):text.index(tool.END) + len(tool.END)] == tool.block()      # what `tools/noise_table.py --check` compares


CORNER_ROWS = [(0, 0), (1, 0), (0, 1), (MAX_A, 0), (0, MAX_B), (MAX_A, MAX_B), (MAX_A - 1, MAX_B - 1), (4 * 4 * 65536, 32768), (65535, 65537),
               (3 * 3 * 65536 - 1, 1), (3 * 3 * 65536, 0)]


def test_isqrt_is_exact_on_the_corner_rows():
    for a, b in CORNER_ROWS:
        x = a + b * np.arange(256, dtype=np.int64)
        s = isqrt(x)
        assert (s * s <= x).all() and ((s + 1) * (s + 1) > x).all(), (a, b)
        assert np.array_equal(s, sigma_table([0, 0, a, b]))
    assert sigma_table([0, 0, MAX_A, MAX_B]).max() == math.isqrt(MAX_A + 255 * MAX_B) == 10026
    assert 3756 * 10026 + (1 << 17) < 2 ** 31                        # the product and the rounding term fit an int32
    assert sigma_table([0, 0, 16 * 65536, 0]).tolist() == [4 * 256] * 256


def test_statistics_of_the_reference():
    """A constant-128 frame of 256 x 256 x 3, key (123, 456): the mean within 0.1 of 128 and the standard deviation within 2 % of
    sqrt(sigma^2 + 1/12) (the 1/12 is the integer rounding) -- more than ten standard errors of 196,608 samples; fixed inputs."""
    img = np.full((256, 256, 3), 128, dtype=np.uint8)
    for (sigma, gain), want in (((4.0, 0.0), 4.010), ((0.0, 0.5), 8.005)):
        row = rows_of([(123, 456, sigma, gain)])[0]
        out = noise_ref(img, row).astype(np.float64)
        assert abs(math.sqrt((sigma * sigma + gain * 128) + 1 / 12) - want) < 1e-3
        print(f"sigma_read {sigma} gain {gain}: mean {out.mean():.4f} std {out.std():.4f} (expected {want})")
        assert abs(out.mean() - 128) < 0.1, out.mean()
        assert abs(out.std() / want - 1) < 0.02, out.std()
        assert out.min() > 0 and out.max() < 255                     # no clamp took part
    # channels and neighbours are independent draws: the correlation of successive bytes is that of noise
    z = unit_normals(196608, (123, 456)).astype(np.float64)
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 0.01 and abs(np.corrcoef(z[:-3], z[3:])[0, 1]) < 0.01


def test_rows_identity_and_clamps():
    rng = np.random.default_rng(5)
    for kind in ("zeros", "full", "ramp", "random"):
        img = noise_image(kind, 9, 11, rng)
        assert np.array_equal(noise_ref(img, [123, 456, 0, 0]), img), kind       # the zero row is the identity, whatever the key
        garbage = noise_ref(img, [7, 9, 0xFFFFFFFF, 0xFFFFFFFF])
        assert np.array_equal(garbage, noise_ref(img, [7, 9, MAX_A, MAX_B])), kind
        assert np.array_equal(garbage, noise_ref(img, [7, 9, -1, -1])), kind     # the int32 pattern of the same words
        assert np.array_equal(noise_ref(img, [7, 9, MAX_A + 1, 0]), noise_ref(img, [7, 9, MAX_A, 0])), kind
        assert (garbage != img).any()
    ramp = noise_image("ramp", 16, 16, rng)
    assert (noise_ref(ramp, [1, 2, 65536, 0]) != noise_ref(ramp, [1, 3, 65536, 0])).any()      # the key matters
    lo, hi = noise_ref(noise_image("zeros", 16, 16, rng), [1, 2, MAX_A, 0]), noise_ref(noise_image("full", 16, 16, rng), [1, 2, MAX_A, 0])
    assert (lo == 0).sum() > 300 and (lo > 0).any() and (hi == 255).sum() > 300 and (hi < 255).any()      # both clamps take part


def test_noise_rows_rounding_and_wrapping():
    from structuredetector_amd.data import noise_rows
    assert noise_rows([(1, 2, 0.0, 0.0)]) == [[1, 2, 0, 0]]
    assert noise_rows([(123, 456, 4.0, 0.5)]) == [[123, 456, 16 * 65536, 32768]]
    assert noise_rows([(0, 0, 32.0, 2.0)]) == [[0, 0, MAX_A, MAX_B]]
    assert noise_rows([(2 ** 32 - 1, 2 ** 31, 0.0, 0.0)]) == [[-1, -2 ** 31, 0, 0]]                 # keys wrap to int32 bit patterns
    assert noise_rows([(2 ** 31 - 1, 2 ** 31 + 5, 0.0, 0.0)]) == [[2 ** 31 - 1, -2 ** 31 + 5, 0, 0]]
    s, g = 1.2345, 0.0123
    assert noise_rows([(5, 6, s, g)]) == [[5, 6, round(s * s * 65536.0), round(g * 65536.0)]]
    assert noise_rows([(5, 6, 200.0, 0.0)]) == [[5, 6, ((200 * 200 * 65536) & 0xFFFFFFFF) - 2 ** 32, 0]]      # beyond int32: wrapped, then clamped by the stage
    rows = noise_rows(iter([(1, 2, 0.5, 0.25), (3, 4, 0.0, 1.0)]))                                 # any iterable
    assert rows == [[1, 2, 16384, 16384], [3, 4, 0, 65536]]
    for row, ref in zip(noise_rows([(9, 8, 3.3, 0.7)]), rows_of([(9, 8, 3.3, 0.7)])):
        assert [v & 0xFFFFFFFF for v in row] == ref


def test_flags_parse_default_to_off_and_are_range_checked():
    from structuredetector_amd.utils.args import Arguments, check_aug_noise
    parser = Arguments().parser
    ns = parser.parse_args([])
    assert (ns.aug_noise, ns.aug_noise_shot) == (0.0, 0.0)
    ns = parser.parse_args(["--aug_noise", "6", "--aug_noise_shot", "0.5"])
    assert (ns.aug_noise, ns.aug_noise_shot) == (6.0, 0.5)
    assert check_aug_noise(ns) == (6.0, 0.5)
    text = " ".join(parser.format_help().split())
    assert "--aug_noise R" in text and "--aug_noise_shot G" in text and "Philox" in text and "not --synthetic" in text
    for flag, bad in (("--aug_noise", "-0.1"), ("--aug_noise", "32.5"), ("--aug_noise", "nan"), ("--aug_noise_shot", "-1"),
                      ("--aug_noise_shot", "2.01"), ("--aug_noise_shot", "nan")):
        with pytest.raises(AssertionError, match=f"'{flag[2:]}'"):
            Arguments().parse([f"{flag}={bad}"])
    assert check_aug_noise(parser.parse_args([])) == (0.0, 0.0)
    assert check_aug_noise(Namespace()) == (0.0, 0.0)                                   # a namespace from before the flags
    assert check_aug_noise(parser.parse_args(["--synthetic", "8"])) == (0.0, 0.0)       # off: --synthetic is fine
    assert check_aug_noise(Namespace(aug_noise=32, aug_noise_shot=2)) == (32.0, 2.0)
    for bad in (dict(aug_noise=-0.5), dict(aug_noise=32.01), dict(aug_noise=float("nan")), dict(aug_noise="4"), dict(aug_noise=True),
                dict(aug_noise_shot=3), dict(aug_noise_shot=-0.1), dict(aug_noise_shot=float("nan")), dict(aug_noise_shot="1")):
        with pytest.raises(ValueError, match=f"'{next(iter(bad))}'"):
            check_aug_noise(Namespace(**bad))
    for on in (["--aug_noise", "4"], ["--aug_noise_shot", "0.5"]):                      # either flag alone switches the stage on
        with pytest.raises(ValueError, match="need --train_dir, not --synthetic"):
            check_aug_noise(parser.parse_args(on + ["--synthetic", "8"]))
        from structuredetector_amd.model.trainer import Trainer
        with pytest.raises(ValueError, match="'aug_noise' / 'aug_noise_shot' work on source images"):   # `train` checks before it builds anything
            Trainer(parser.parse_args(on + ["--synthetic", "8"]))


_COMMON = dict(width=128, height=128, no_augmentation=False, aug_rotate=10.0, aug_mosaic=0.5, aug_transpose=0.5, train_tiles="2x2", tile_overlap=32,
               aug_blur=2.0, aug_perspective=0.3, aug_jpeg=30, aug_equalize=0.3, aug_autocontrast=0.6, aug_autocontrast_cutoff=5.0, device="cpu")


def _expected(u, keys, read, shot):
    return [(k0, k1, u1 * read, u2 * shot) if u0 < 0.5 else (k0, k1, 0.0, 0.0) for (u0, u1, u2), (k0, k1) in zip(u, keys)]


def test_no_draw_when_off_and_exactly_two_draws_when_on():
    from structuredetector_amd.data import TrainAugmentation, ValidationAugmentation, noise_rows
    for extra in (dict(), dict(aug_noise=0.0, aug_noise_shot=0.0), dict(aug_noise=6.0, aug_noise_shot=0.5, no_augmentation=True)):
        aug = TrainAugmentation(Namespace(**{**_COMMON, **extra}))
        torch.manual_seed(3)
        before = torch.get_rng_state()
        assert aug.noise_draws_for(6) is None
        assert torch.equal(torch.get_rng_state(), before), extra                        # no draw at all
    val = ValidationAugmentation(Namespace(width=128, height=96, aug_noise=6.0, aug_noise_shot=1.0))
    before = torch.get_rng_state()
    assert val.noise_draws_for(6) is None and torch.equal(torch.get_rng_state(), before)
    for read, shot in ((6.0, 0.5), (32.0, 0.0), (0.0, 2.0)):                            # either flag alone switches the stage on
        aug = TrainAugmentation(Namespace(**_COMMON, aug_noise=read, aug_noise_shot=shot))
        torch.manual_seed(3)
        draws = aug.noise_draws_for(256)
        torch.manual_seed(3)
        u = torch.rand(256, 3, dtype=torch.float64).tolist()                            # the two draws, in this order
        keys = torch.randint(0, 2 ** 32, (256, 2), dtype=torch.int64).tolist()
        after = torch.get_rng_state()
        assert draws == _expected(u, keys, read, shot)
        torch.manual_seed(3)
        aug.noise_draws_for(256)
        assert torch.equal(torch.get_rng_state(), after)
        on = [d for d in draws if d[2] > 0 or d[3] > 0]
        assert 80 < len(on) < 176 and all(0 <= d[2] <= read and 0 <= d[3] <= shot for d in draws)
        assert len({d[:2] for d in draws}) == 256 and max(d[0] for d in draws) >= 2 ** 31          # distinct keys over the whole 32 bits
        rows = noise_rows(draws)
        assert all(-2 ** 31 <= v < 2 ** 31 for r in rows for v in r)


def test_the_draws_come_after_the_tone_draw_and_change_no_earlier_one():
    """The draws `__call__` makes, in its order: with the flags off the generator ends where the parent's does; with them on every earlier
    draw is the same and the next numbers of the generator are the noise draws'."""
    from structuredetector_amd.data import TrainAugmentation
    seen, ends = [], []
    n, groups = 8, [[0, 1, 2, 3], [4, 5, 6, 7]]
    for flags in (dict(), dict(aug_noise=0.0, aug_noise_shot=0.0), dict(aug_noise=6.0, aug_noise_shot=0.5)):
        aug = TrainAugmentation(Namespace(**_COMMON, **flags))
        torch.manual_seed(11)
        seen.append((aug.draws_for(n), aug.affine_draws_for(n), aug.mosaic_draws_for(n, groups), aug.window_draws_for(n), aug.transpose_draws_for(n),
                     aug.blur_draws_for(n), aug.perspective_draws_for(n), aug.jpeg_draws_for(n), aug.tone_draws_for(n)))
        assert seen[-1][-1] is not None
        state = torch.get_rng_state()
        tail = aug.noise_draws_for(n)
        ends.append(torch.get_rng_state())
        assert (tail is None) == (not flags.get("aug_noise"))
        if tail is None:
            assert torch.equal(ends[-1], state)
        else:
            torch.set_rng_state(state)
            u = torch.rand(n, 3, dtype=torch.float64).tolist()
            keys = torch.randint(0, 2 ** 32, (n, 2), dtype=torch.int64).tolist()
            assert tail == _expected(u, keys, 6.0, 0.5) and torch.equal(torch.get_rng_state(), ends[-1])
    assert seen[0] == seen[1] == seen[2] and torch.equal(ends[0], ends[1]) and not torch.equal(ends[0], ends[2])


def test_the_call_makes_the_draws_in_that_order(monkeypatch):
    """`ValidationAugmentation.__call__` asks for the noise draws last: DRAW_STEPS, the one place the order is written, names the draw
    functions in the order of the test above, and the call runs whatever is bound to those names, in that order, once each."""
    from structuredetector_amd.data import augment as A
    from structuredetector_amd.utils import ImageAnnotation
    names = ("draws_for", "affine_draws_for", "mosaic_draws_for", "window_draws_for", "transpose_draws_for", "blur_draws_for",
             "perspective_draws_for", "jpeg_draws_for", "tone_draws_for", "noise_draws_for")
    assert A.DRAW_STEPS == names
    aug, asked = A.TrainAugmentation(Namespace(**_COMMON, aug_noise=6.0)), []
    for name in names:
        real = getattr(aug, name)
        setattr(aug, name, lambda *a, name=name, real=real: asked.append(name) or real(*a))
    monkeypatch.setattr(A, "preprocess_images", lambda images, size, **kw: torch.zeros(images.shape[0], 3, size[1], size[0]))
    monkeypatch.setattr(A, "transpose_select", lambda batch, select: batch)
    out, _ = aug([np.zeros((40, 56, 3), np.uint8)] * 4, [ImageAnnotation(f"/i{i}.png") for i in range(4)])
    assert asked == list(names) and out.shape == (4, 3, 128, 128)


NAMES = ["sd_noise_normal_table", "sd_noise_u8", "sd_preprocess_noise_workspace_bytes", "sd_preprocess_images_noise",
         "sd_preprocess_images_list_noise"]


def test_header_declares_and_the_library_exports_the_noise_symbols():
    from structuredetector_amd import _lib as L
    header = (ROOT / "include" / "sdnet_hip.h").read_text()
    for name in NAMES:
        assert re.search(rf"^(size_t|int) {name}\(", header, re.M), name
    handle = L.lib()
    assert set(NAMES) <= set(L.declared_symbols())
    assert all(hasattr(handle, n) for n in NAMES)
    for geometry, g in ((0, (0, 0)), (1, (0, 30)), (2, (32, 0))):                       # the tone form's size: the stage needs no workspace
        for out in ((32, 32), (33, 31)):
            args = (geometry, 4, 40, 56, g[0], *out, g[1])
            assert handle.sd_preprocess_noise_workspace_bytes(*args) == handle.sd_preprocess_tone_workspace_bytes(*args) > 0


def test_sd_noise_u8_rejects_bad_arguments_without_touching_the_gpu():
    """Every bad call returns before a launch (the pointers are never dereferenced) and sd_last_error() names the function."""
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def call(src=16, dst=1 << 20, B=2, H=5, W=7, table=2 << 20):
        return lib.sd_noise_u8(src, dst, B, H, W, table, 0)

    for kw, text in [(dict(src=0), "null"), (dict(dst=0), "null"), (dict(table=0), "null"), (dict(B=0), "bad shape"), (dict(H=0), "bad shape"),
                     (dict(W=-16), "bad shape"), (dict(B=-1), "bad shape"), (dict(B=65536), "65535"), (dict(H=65536, W=32768), "2^31"),
                     (dict(dst=16 + 48), "overlap"), (dict(dst=16 - 1, src=16 + 7), "overlap")]:
        assert call(**kw) == -1, kw                                  # SD_ERR_INVALID
        msg = lib.sd_last_error().decode()
        assert "sd_noise_u8" in msg and text in msg, (kw, msg)
