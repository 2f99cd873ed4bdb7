"""Gaussian blur augmentation (`--aug_blur`), the parts that need no GPU: tests/blur_ref.py against Pillow itself byte for byte, the host's
`blur_box_params` against the reference's table, SD_BLUR_MAX_RADIUS against the largest legal radius, the flag and its refusals, the extra
training draw, and the argument validation of `sd_blur_u8` (host code that runs before any launch)."""
import re
from argparse import Namespace
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.blur_ref import blur_ref, box_params

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(1, 1), (2, 3), (5, 7), (3, 40), (33, 17), (64, 96), (130, 70)]                  # (height, width)
RADII = [0.1, 0.3, 0.5, 0.7, 1.0, 1.5, 2.5, 3.3, 5, 8]


@pytest.mark.parametrize("shape", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_blur_ref_is_pillow_byte_for_byte(shape):
    """Zero mismatches: random images and images of only 0 / 255, both orientations of every size, every radius."""
    from PIL import Image, ImageFilter
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    for h, w in {shape, shape[::-1]}:
        images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)]
        for r in RADII:
            for k, a in enumerate(images):
                want = np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(r)))
                got = blur_ref(a, r)
                assert np.array_equal(got, want), f"{h}x{w} r={r} image {k}: {(got != want).sum()} bytes differ"
    a = rng.integers(0, 256, (shape[0], shape[1], 3), dtype=np.uint8)
    assert np.array_equal(blur_ref(a, 0), a)
    assert np.array_equal(np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(0))), a)


def test_box_params_are_the_float32_values_the_issue_pins():
    assert box_params(1.0) == (0, 11184811, 2796202)                                    # the float32 quotient: double gives ww = 11184810
    assert box_params(0.3)[0] == 0 and box_params(0.3)[2] > 0                           # R = 0: the edge weight alone
    for r in RADII:
        R, ww, fw = box_params(r)
        assert 0 <= R and ww > 0 and fw >= 0 and (2 * R + 1) * ww + 2 * fw <= 1 << 24    # the uint32 sum of a pass never wraps


def test_blur_box_params_equals_the_reference_table():
    from structuredetector_amd.data import blur_box_params
    for r in [*RADII, 2.0, 7.999, *np.linspace(0.001, 8, 1601)]:
        assert blur_box_params(r) == box_params(r), r
    assert blur_box_params(0) == blur_box_params(0.0) == (0, 1 << 24, 0)                # r = 0: the copy row
    for bad in (-0.1, 8.01, float("nan")):
        with pytest.raises(ValueError, match="blur radius"):
            blur_box_params(bad)


def test_max_radius_is_computed_from_the_largest_legal_flag():
    from structuredetector_amd.utils.args import MAX_AUG_BLUR
    header = (ROOT / "include" / "sdnet_hip.h").read_text()
    declared = int(re.search(r"#define\s+SD_BLUR_MAX_RADIUS\s+(\d+)", header).group(1))
    assert declared == box_params(MAX_AUG_BLUR)[0] == 7
    assert max(box_params(r)[0] for r in np.linspace(0.001, MAX_AUG_BLUR, 4001)) == declared       # the box radius grows with r


def test_flag_parses_defaults_to_off_and_is_range_checked():
    from structuredetector_amd.utils.args import Arguments, check_aug_blur
    parser = Arguments().parser
    assert parser.parse_args([]).aug_blur == 0.0
    assert parser.parse_args(["--aug_blur", "2.5"]).aug_blur == 2.5
    text = " ".join(parser.format_help().split())
    assert "--aug_blur R" in text and "GaussianBlur" in text and "not --synthetic" in text
    for bad in ("-0.5", "8.5"):
        with pytest.raises(AssertionError, match="aug_blur"):
            Arguments().parse(["--aug_blur", bad])
    assert check_aug_blur(parser.parse_args([])) == 0.0
    assert check_aug_blur(Namespace()) == 0.0                                           # a namespace from before the flag
    assert check_aug_blur(parser.parse_args(["--aug_blur", "8"])) == 8.0
    assert check_aug_blur(parser.parse_args(["--synthetic", "8"])) == 0.0               # off: --synthetic is fine
    for bad in (-1.0, 8.5, float("nan")):
        with pytest.raises(ValueError, match="aug_blur"):
            check_aug_blur(Namespace(aug_blur=bad))
    with pytest.raises(ValueError, match="'aug_blur' blurs source images: it needs --train_dir, not --synthetic"):
        check_aug_blur(parser.parse_args(["--aug_blur", "2", "--synthetic", "8"]))
    from structuredetector_amd.model.trainer import Trainer
    with pytest.raises(ValueError, match="needs --train_dir, not --synthetic"):         # `train` checks before it builds anything (no GPU is touched)
        Trainer(parser.parse_args(["--aug_blur", "2", "--synthetic", "8"]))


_COMMON = dict(width=128, height=96, no_augmentation=False, aug_rotate=10.0, aug_mosaic=0.5, aug_transpose=0.0, train_tiles="", device="cpu")


def test_no_draw_when_off_and_one_draw_when_on():
    from structuredetector_amd.data import TrainAugmentation, ValidationAugmentation
    for extra in (dict(), dict(aug_blur=0.0), dict(aug_blur=0), dict(aug_blur=2.0, no_augmentation=True)):
        aug = TrainAugmentation(Namespace(**{**_COMMON, **extra}))
        torch.manual_seed(3)
        before = torch.get_rng_state()
        assert aug.blur_draws_for(6) is None
        assert torch.equal(torch.get_rng_state(), before), extra                        # no draw at all
    val = ValidationAugmentation(Namespace(width=128, height=96, aug_blur=2.0))
    before = torch.get_rng_state()
    assert val.blur_draws_for(6) is None and torch.equal(torch.get_rng_state(), before)
    aug = TrainAugmentation(Namespace(**_COMMON, aug_blur=2.0))
    torch.manual_seed(3)
    radii = aug.blur_draws_for(64)
    torch.manual_seed(3)
    u = torch.rand(64, 2, dtype=torch.float64).tolist()                                 # ONE draw: rand(n, 2) in float64
    after = torch.get_rng_state()
    assert radii == [2.0 * u1 if u0 < 0.5 else 0.0 for u0, u1 in u]
    torch.manual_seed(3)
    aug.blur_draws_for(64)
    assert torch.equal(torch.get_rng_state(), after)
    assert any(r == 0.0 for r in radii) and any(r > 0 for r in radii) and all(0 <= r <= 2.0 for r in radii)


def test_earlier_draws_of_a_batch_do_not_depend_on_the_flag():
    """The blur draw comes last: flips, jitter, warp, mosaic, window and transpose draws are the same with the flag on and off."""
    from structuredetector_amd.data import TrainAugmentation
    common = {**_COMMON, "width": 128, "height": 128, "aug_transpose": 0.5, "train_tiles": "2x2", "tile_overlap": 32}
    seen = []
    for blur in (0.0, 2.0):
        aug = TrainAugmentation(Namespace(**common, aug_blur=blur))
        torch.manual_seed(11)
        n, groups = 8, [[0, 1, 2, 3], [4, 5, 6, 7]]
        seen.append((aug.draws_for(n), aug.affine_draws_for(n), aug.mosaic_draws_for(n, groups), aug.window_draws_for(n), aug.transpose_draws_for(n)))
        tail = aug.blur_draws_for(n)
        assert (tail is None) == (blur == 0.0)
    assert seen[0] == seen[1]


def test_library_exports_the_blur_symbols():
    from structuredetector_amd import _lib as L
    handle = L.lib()
    names = {"sd_blur_u8", "sd_blur_workspace_bytes", "sd_preprocess_images_blur", "sd_preprocess_images_list_blur",
             "sd_preprocess_blur_workspace_bytes"}
    assert names <= set(L.declared_symbols())
    assert all(hasattr(handle, n) for n in names)
    assert handle.sd_blur_workspace_bytes(2, 5, 7) == 256                               # 210 bytes, rounded up to 256
    # the chain's workspace is that of the geometry's own entry point with every stage on
    assert handle.sd_preprocess_blur_workspace_bytes(0, 4, 40, 56, 0, 32, 32, 0) == handle.sd_preprocess_mosaic_workspace_bytes(4, 40, 56, 32, 32)
    assert handle.sd_preprocess_blur_workspace_bytes(1, 4, 40, 56, 0, 32, 32, 30) == handle.sd_preprocess_window_workspace_bytes(4, 30, 32, 32)
    assert handle.sd_preprocess_blur_workspace_bytes(2, 4, 40, 56, 32, 32, 32, 0) == handle.sd_preprocess_letterbox_workspace_bytes(4, 40, 32, 32, 32)


def test_sd_blur_u8_rejects_bad_arguments_without_touching_the_gpu():
    """Every bad call returns before a launch (the pointers are never dereferenced) and sd_last_error() names the function."""
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def call(src=16, dst=1 << 20, B=2, H=5, W=7, blur=2 << 20, ws=3 << 20, ws_bytes=256):
        return lib.sd_blur_u8(src, dst, B, H, W, blur, ws, ws_bytes, 0)

    for kw, text in [(dict(src=0), "null"), (dict(dst=0), "null"), (dict(blur=0), "null"), (dict(ws=0), "null"), (dict(dst=16), "in place"),
                     (dict(B=0), "bad shape"), (dict(H=0), "bad shape"), (dict(W=-1), "bad shape"), (dict(B=70000), "too large"),
                     (dict(ws_bytes=255), "workspace 255 < 256")]:
        assert call(**kw) != 0, kw
        msg = lib.sd_last_error().decode()
        assert "sd_blur_u8" in msg and text in msg, (kw, msg)
