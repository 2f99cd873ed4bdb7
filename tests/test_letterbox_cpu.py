"""Aspect-preserving input (`--keep_aspect`), host side: the geometry on the shared cases and over a sweep of small sizes, the annotation
round trip, the flag and its refusals, and the argument checks of sd_preprocess_images_letterbox / _list_letterbox (they return before any
launch)."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest

from tests.letterbox_ref import CASES, FILL, geometry, pil_frame, sources


def test_geometry_on_the_shared_cases_and_the_issue_table():
    from structuredetector_amd.data.augment import _FILL, letterbox_geometry
    from structuredetector_amd.utils.misc import letterbox_geometry as from_misc
    assert letterbox_geometry is from_misc and tuple(_FILL) == FILL
    for (hin, win), frame, listed in CASES:
        got = letterbox_geometry((win, hin), frame)
        assert got == geometry((hin, win), frame), ((hin, win), frame)
        if listed is not None:
            assert got == listed, ((hin, win), frame)
    assert letterbox_geometry((30, 20), (96, 64)) == (96, 64, 0, 0)            # upscale, exact fit
    assert letterbox_geometry((37, 23), (64, 32)) == (51, 32, 6, 0)            # the landscape twin of the first case: 37 * 32 / 23 = 51.48
    assert letterbox_geometry((1, 300), (64, 32)) == (1, 32, 31, 0)            # one inner column
    assert letterbox_geometry((2448, 2048), (512, 512)) == (512, 428, 0, 42)   # the camera frame
    with pytest.raises(ValueError):
        letterbox_geometry((0, 5), (64, 64))


def test_geometry_properties_over_a_sweep_of_small_sizes():
    from structuredetector_amd.data.augment import letterbox_geometry
    sides = list(range(1, 14)) + [31, 32, 33, 64, 100]
    frames = [(w, h) for w in (1, 2, 5, 8, 32, 33) for h in (1, 3, 8, 32)]
    for win in sides:
        for hin in sides:
            for W, H in frames:
                wi, hi, px, py = letterbox_geometry((win, hin), (W, H))
                assert 1 <= wi <= W and 1 <= hi <= H, (win, hin, W, H)
                assert wi == W or hi == H                                       # the frame is covered on at least one axis
                assert (px, py) == ((W - wi) // 2, (H - hi) // 2) and px + wi <= W and py + hi <= H
                assert (hi, wi, py, px) == letterbox_geometry((hin, win), (H, W))   # symmetric under swapping the axes
                if wi == W and hi < H:                                          # the free side is the nearest integer to the exact height
                    assert abs(hi * win - hin * W) * 2 <= win or hi == 1
                if win * H == hin * W:
                    assert (wi, hi) == (W, H)                                   # same aspect ratio: no bars


def test_pillow_frame_is_the_resized_image_between_bars_of_fill():
    """The definition the kernels are pinned to, spelled out once on the host: inside the rectangle Pillow's plain resize, outside FILL."""
    from PIL import Image
    for src, frame, _ in CASES:
        img = sources(src, n=1)[0]
        wi, hi, px, py = geometry(src, frame)
        f = pil_frame(img, frame)
        assert f.shape == (frame[1], frame[0], 3)
        assert np.array_equal(f[py:py + hi, px:px + wi], np.asarray(Image.fromarray(img).resize((wi, hi), Image.BILINEAR)))
        mask = np.ones(f.shape[:2], bool)
        mask[py:py + hi, px:px + wi] = False
        assert (f[mask] == np.asarray(FILL, np.uint8)).all()


def test_annotation_letterbox_then_unletterbox_returns_the_keypoints():
    from structuredetector_amd.utils import Box, ImageAnnotation, Keypoint, Object
    from structuredetector_amd.utils.misc import letterbox_annotation, letterbox_geometry, unletterbox_annotation
    rng = np.random.default_rng(7)
    for (hin, win), frame, _ in CASES + [((2048, 2448), (512, 512), None), ((333, 61), (128, 64), None)]:
        pts = [(float(rng.uniform(0, win - 1)), float(rng.uniform(0, hin - 1))) for _ in range(6)] + [(0.0, 0.0), (win - 1.0, hin - 1.0)]
        ann = ImageAnnotation("a.png", [Object("bean", Keypoint("stem", x, y), [Keypoint("leaf", y * (win - 1) / max(hin - 1, 1), x * (hin - 1) / max(win - 1, 1))],
                                               Box(x / 2, y / 2, x, y)) for x, y in pts], img_size=(win, hin))
        orig = ann.clone()
        wi, hi, px, py = letterbox_geometry((win, hin), frame)
        letterbox_annotation(ann, (win, hin), frame)
        assert len(ann.objects) == len(pts)                                     # nothing leaves the frame
        for o, q in zip(ann.objects, orig.objects):
            assert abs(o.x - (q.x * (wi / win) + px)) <= 1e-9 and abs(o.y - (q.y * (hi / hin) + py)) <= 1e-9
            assert px <= o.x < px + wi and py <= o.y < py + hi                  # inside the placed image, so inside the frame
        unletterbox_annotation(ann, (win, hin), frame)
        tol = 1e-12 * max(win, hin) * max(win / wi, hin / hi)                   # fp64 rounding of a shift of a frame coordinate, scaled back
        for o, q in zip(ann.objects, orig.objects):
            for a, b in [(o.anchor, q.anchor), (o.parts[0], q.parts[0])]:
                assert abs(a.x - b.x) <= tol and abs(a.y - b.y) <= tol, ((hin, win), frame)
            for k in ("x_min", "x_max", "y_min", "y_max"):
                assert abs(getattr(o.box, k) - getattr(q.box, k)) <= tol


def test_keep_aspect_flag_parses_and_refuses_what_it_cannot_combine_with():
    from structuredetector_amd.utils.args import Arguments, check_keep_aspect
    parser = Arguments().parser
    ns = parser.parse_args([])
    assert ns.keep_aspect is False and check_keep_aspect(ns) is False and check_keep_aspect(ns, training=True) is False
    assert check_keep_aspect(Namespace()) is False                              # a namespace from before the flag
    ns = parser.parse_args(["--keep_aspect"])
    assert ns.keep_aspect is True and check_keep_aspect(ns) is True and check_keep_aspect(ns, training=True) is True
    # every option that works on the frame or after it combines
    ok = parser.parse_args(["--keep_aspect", "--tta", "hvflip", "--tta_transpose", "--label_nms", "2", "--pr_curve", "--cache_images", "0.5",
                            "--bf16_inference", "--aug_rotate", "10", "--aug_mosaic", "0.5", "--amp"])
    assert check_keep_aspect(ok) is True and check_keep_aspect(ok, training=True) is True
    with pytest.raises(ValueError, match="'keep_aspect' does not combine with --tiles"):
        check_keep_aspect(parser.parse_args(["--keep_aspect", "--tiles", "2x2"]))
    with pytest.raises(ValueError, match="'keep_aspect' does not combine with --tta_scales"):
        check_keep_aspect(parser.parse_args(["--keep_aspect", "--tta_scales", "0.75"]))
    with pytest.raises(ValueError, match="'keep_aspect' does not combine with --train_tiles"):
        check_keep_aspect(parser.parse_args(["--keep_aspect", "--train_tiles", "2x2"]), training=True)
    for training in (False, True):
        with pytest.raises(ValueError, match="'keep_aspect' letterboxes source images.*--synthetic"):
            check_keep_aspect(parser.parse_args(["--keep_aspect", "--synthetic", "8"]), training=training)
    # train never consults --tiles / --tta_scales, evaluate and detect never --train_tiles; off or 1x1 is no tiling
    assert check_keep_aspect(parser.parse_args(["--keep_aspect", "--tiles", "2x2", "--tta_scales", "0.75"]), training=True) is True
    assert check_keep_aspect(parser.parse_args(["--keep_aspect", "--train_tiles", "2x2"])) is True
    assert check_keep_aspect(parser.parse_args(["--keep_aspect", "--tiles", "1x1"])) is True
    # without the flag nothing is refused here
    assert check_keep_aspect(parser.parse_args(["--tiles", "2x2", "--tta_scales", "0.75", "--synthetic", "8"])) is False
    # the entry points check before they build anything (no GPU is touched)
    from structuredetector_amd.model.predictor import Predictor
    from structuredetector_amd.model.trainer import Trainer
    with pytest.raises(ValueError, match="--train_tiles"):
        Trainer(parser.parse_args(["--keep_aspect", "--train_tiles", "2x2", "--tile_overlap", "64", "--train_dir", "x"]))
    with pytest.raises(ValueError, match="--synthetic"):
        Trainer(parser.parse_args(["--keep_aspect", "--synthetic", "8"]))
    with pytest.raises(ValueError, match="--tiles"):
        Predictor(parser.parse_args(["--keep_aspect", "--tiles", "2x2", "-o", "w.pth"]))
    text = " ".join(parser.format_help().split())
    assert "--keep_aspect" in text and "letterbox" in text and "--tta_scales" in text


def test_augmentations_read_the_flag_and_it_draws_nothing():
    import torch

    from structuredetector_amd.data.augment import TrainAugmentation, ValidationAugmentation
    assert ValidationAugmentation(Namespace(width=128, height=64)).keep_aspect is False
    assert ValidationAugmentation(Namespace(width=128, height=64, keep_aspect=True)).keep_aspect is True
    groups = [[0, 1, 2], [3, 4, 5]]
    states = []
    for flag in (False, True):                                                  # the draw sequence with the flag on is the one with it off
        aug = TrainAugmentation(Namespace(width=128, height=64, no_augmentation=False, aug_scale=0.2, aug_mosaic=0.5, keep_aspect=flag))
        assert aug.keep_aspect is flag
        torch.manual_seed(5)
        drawn = (aug.draws_for(6), aug.affine_draws_for(6), aug.mosaic_draws_for(6, groups), aug.window_draws_for(6), aug.transpose_draws_for(6))
        states.append((drawn, torch.get_rng_state()))
    assert states[0][0] == states[1][0] and torch.equal(states[0][1], states[1][1])


def test_c_abi_rejects_bad_geometry_before_any_launch():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    Bn, Hin, Win, Hi, Wi, Hout, Wout, y0, x0 = 2, 16, 30000, 8, 40, 12, 64, 2, 12
    need = lib.sd_preprocess_letterbox_workspace_bytes(Bn, Hin, Wi, Hout, Wout)
    assert need >= Bn * Hin * Wi * 3 + 2 * Bn * Hout * Wout * 3 + Bn * 8
    m3, s3, fill = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25), (C.c_ubyte * 3)(*FILL)
    P = 4096                                                                   # never dereferenced: no call below reaches a launch
    for fn, name, is_list in ((lib.sd_preprocess_images_letterbox, b"sd_preprocess_images_letterbox", False),
                              (lib.sd_preprocess_images_list_letterbox, b"sd_preprocess_images_list_letterbox", True)):
        def call(win=100, hi=Hi, wi=Wi, y=y0, x=x0, order=None, factors=None, affine=None, geom=None, mats=None, fill3=fill, ws=need):
            return fn(P, Bn, Hin, win, hi, wi, Hout, Wout, y, x, P, P, 3, P, P, 3, None, order, factors, affine, geom, mats, fill3, m3, s3, P, P,
                      ws, 0)
        cases = [("a negative x origin", dict(x=-1), -1), ("a negative y origin", dict(y=-1), -1),
                 ("an inner image past the right edge", dict(x=Wout - Wi + 1), -1), ("an inner image past the bottom edge", dict(y=Hout - Hi + 1), -1),
                 ("an inner image wider than the frame", dict(wi=Wout + 1, x=0), -1), ("an inner image of no rows", dict(hi=0), -1),
                 ("a null fill colour", dict(fill3=None), -1), ("a null fill colour with a warp", dict(affine=P, fill3=None), -1),
                 ("a jitter table alone", dict(order=P), -1), ("jitter factors alone", dict(factors=P), -1),
                 ("mosaic geometry alone", dict(geom=P), -1), ("mosaic matrices alone", dict(mats=P), -1),
                 ("a workspace one byte short", dict(ws=need - 1), -2)]
        if is_list:
            cases.append(("source rows over the LDS limit", dict(win=Win), -1))
        for what, kw, code in cases:
            lib.sd_set_option(b"no_such_option", 1)                            # leaves another message behind
            assert call(**kw) == code, f"{name.decode()}: {what}"
            assert lib.sd_last_error() and name in lib.sd_last_error(), f"{name.decode()}: {what}: {lib.sd_last_error()}"
    assert b"LDS" in lib.sd_last_error() and b"21834" in lib.sd_last_error()
