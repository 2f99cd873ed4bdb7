"""Crop training at the tile scale (`train --train_tiles`), host side: the window extents against a brute force, Pillow's cropped resize
against the slice of its full resize on the project's tables, the flags, the draws, the annotation rule, and the argument checks of
sd_preprocess_images_window / _list_window (they return before any launch)."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.affine_ref import FILL
from tests.window_ref import brute_extent, pil_window, sources


def test_window_extents_match_a_brute_force_and_the_camera_frame_case():
    from structuredetector_amd.data.augment import window_extents
    from structuredetector_amd.utils.args import tile_canvas
    assert tile_canvas(512, 512, (3, 3), 64) == (1408, 1408)
    assert window_extents(2448, 1408, 512) == 892 and window_extents(2048, 1408, 512) == 747        # 2448 x 2048 frame, 3x3 tiles of 512
    for in_size, canvas, out in ((201, 96, 64), (150, 96, 64), (50, 96, 64), (40, 96, 64), (96, 96, 64), (333, 160, 64), (61, 96, 48),
                                 (333, 128, 64), (61, 64, 48), (6000, 64, 64), (8, 64, 64), (7, 5, 5), (5, 7, 1)):
        assert window_extents(in_size, canvas, out) == brute_extent(in_size, canvas, out), (in_size, canvas, out)
        assert 1 <= window_extents(in_size, canvas, out) <= in_size
    assert window_extents(2448, 1408, 512) == 892                                                     # (cached)
    for bad in ((10, 8, 9), (10, 8, 0)):
        with pytest.raises(ValueError):
            window_extents(*bad)


@pytest.mark.parametrize("hin,win,wc,hc", [(150, 201, 96, 96), (40, 50, 96, 96), (96, 96, 96, 96), (61, 333, 160, 96)])
def test_pillows_cropped_resize_is_the_slice_of_its_full_resize_and_the_tables_are_monotone(hin, win, wc, hc):
    """The definition the kernels are pinned to: the canvas tables indexed at x0 + x, y0 + y."""
    from PIL import Image

    from structuredetector_amd.data.augment import pil_bilinear_coeffs
    img = sources((hin, win), n=1)[0]
    full = np.asarray(Image.fromarray(img).resize((wc, hc), Image.BILINEAR))
    for x0, y0 in ((0, 0), (wc - 64, hc - 48), (wc - 64, 0), (0, hc - 48), ((wc - 64) // 2 | 1 if wc > 64 else 0, (hc - 48) // 2 | 1)):
        assert np.array_equal(pil_window(img, (wc, hc), (x0, y0), (64, 48)), full[y0:y0 + 48, x0:x0 + 64]), (x0, y0)
    for n_in, n_out in ((win, wc), (hin, hc)):
        bounds = pil_bilinear_coeffs(n_in, n_out)[0]
        first, end = bounds[:, 0], bounds[:, 0] + bounds[:, 1]
        assert (np.diff(first) >= 0).all() and (np.diff(end) >= 0).all() and first[0] == 0 and end[-1] == n_in and (bounds[:, 1] >= 1).all()
    if (hin, win) == (hc, wc):                                                  # an identity-size resize through the tables returns the bytes
        assert np.array_equal(full, img)


def test_train_tiles_flag_parses_checks_the_overlap_and_refuses_synthetic():
    from structuredetector_amd.utils.args import Arguments, check_train_tiles, parse_tiles
    parser = Arguments().parser
    ns = parser.parse_args([])
    assert ns.train_tiles == "" and check_train_tiles(ns) == ()
    ns = parser.parse_args(["--train_tiles", "3x2", "--tile_overlap", "32"])
    assert ns.train_tiles == "3x2" and ns.tiles == "" and check_train_tiles(ns) == (3, 2)          # --tiles stays off: train never consults it
    assert check_train_tiles(parser.parse_args(["--train_tiles", "1x1"])) == ()
    assert check_train_tiles(Namespace(train_tiles=(2, 2), width=512, height=512, tile_overlap=64)) == (2, 2)     # an already finalized namespace
    with pytest.raises(ValueError, match="'train_tiles' should be COLUMNSxROWS"):
        check_train_tiles(parser.parse_args(["--train_tiles", "2"]))
    with pytest.raises(ValueError, match="'train_tiles' should have 1 to 8"):
        check_train_tiles(parser.parse_args(["--train_tiles", "9x1"]))
    with pytest.raises(ValueError, match="COLUMNSxROWS"):
        parse_tiles("2")                                                        # (the --tiles message is unchanged)
    # the overlap must hold for the smallest multi-scale size, int(0.75 * side / 32) * 32: 128 -> 96, so 64 > 96 / 2 is refused ...
    with pytest.raises(ValueError, match=r"half the smaller side of 96 x 96"):
        check_train_tiles(parser.parse_args(["--train_tiles", "2x2", "-W", "128", "-H", "128", "--tile_overlap", "64"]))
    assert check_train_tiles(parser.parse_args(["--train_tiles", "2x2", "-W", "128", "-H", "128", "--tile_overlap", "32"])) == (2, 2)
    # ... but accepted when there is no multi-scale (--no_augmentation keeps 128 x 128), and never looked at with the flag off
    assert check_train_tiles(parser.parse_args(["--train_tiles", "2x2", "-W", "128", "-H", "128", "--tile_overlap", "64", "-a"])) == (2, 2)
    assert check_train_tiles(parser.parse_args(["-W", "128", "-H", "128", "--tile_overlap", "48"])) == ()
    with pytest.raises(ValueError, match="multiple of 32"):
        check_train_tiles(parser.parse_args(["--train_tiles", "2x2", "--tile_overlap", "48"]))
    with pytest.raises(ValueError, match="half the smaller side of 384 x 192"):
        check_train_tiles(parser.parse_args(["--train_tiles", "2x2", "-W", "512", "-H", "256", "--tile_overlap", "128"]))
    with pytest.raises(ValueError, match="--synthetic"):
        check_train_tiles(parser.parse_args(["--train_tiles", "2x2", "--synthetic", "8"]))
    from structuredetector_amd.model.trainer import Trainer
    with pytest.raises(ValueError, match="--synthetic"):                        # `train` checks before it builds anything (no GPU is touched)
        Trainer(parser.parse_args(["--train_tiles", "2x2", "--synthetic", "8"]))
    with pytest.raises(ValueError, match="half the smaller side of 96 x 96"):
        Trainer(parser.parse_args(["--train_tiles", "2x2", "-W", "128", "-H", "128", "--train_dir", "x"]))
    text = " ".join(parser.format_help().split())
    assert "--train_tiles CxR" in text and "evaluate --tiles" in text and "--synthetic" in text


def test_window_draws_are_one_more_draw_and_none_with_the_flag_off():
    from structuredetector_amd.data.augment import TrainAugmentation, ValidationAugmentation
    groups = [[0, 1, 2], [3, 4, 5]]
    for extra in (dict(), dict(train_tiles=""), dict(train_tiles="1x1")):
        aug = TrainAugmentation(Namespace(width=128, height=96, no_augmentation=False, aug_scale=0.2, aug_mosaic=0.5, **extra))
        torch.manual_seed(5)
        aug.draws_for(6), aug.affine_draws_for(6), aug.mosaic_draws_for(6, groups)
        state = torch.get_rng_state()                                           # a batch's draws without the feature
        torch.manual_seed(5)
        aug.draws_for(6), aug.affine_draws_for(6), aug.mosaic_draws_for(6, groups)
        assert aug.window_draws_for(6) is None and torch.equal(torch.get_rng_state(), state)
    aug = TrainAugmentation(Namespace(width=128, height=96, no_augmentation=False, train_tiles="3x2", tile_overlap=32))
    torch.manual_seed(6)
    u = torch.rand(4, 2, dtype=torch.float64).tolist()
    state = torch.get_rng_state()
    torch.manual_seed(6)
    canvas, origins = aug.window_draws_for(4)
    assert torch.equal(torch.get_rng_state(), state)                            # exactly rand(n, 2) in float64
    assert canvas == (3 * 128 - 2 * 32, 2 * 96 - 32) == (320, 160)
    assert origins == [(int(ux * (320 - 128 + 1)), int(uy * (160 - 96 + 1))) for ux, uy in u]
    assert all(0 <= x0 <= 192 and 0 <= y0 <= 64 for x0, y0 in origins)
    aug.size = (96, 64)                                                         # the canvas follows the per-epoch multi-scale size
    assert aug.window_draws_for(1)[0] == (3 * 96 - 64, 2 * 64 - 32)
    # --no_augmentation keeps the windows (the flag sets the scale the network is trained at) and draws nothing else
    quiet = TrainAugmentation(Namespace(width=128, height=96, no_augmentation=True, train_tiles="2x2", tile_overlap=32))
    assert quiet.draws_for(3) == (None, None) and quiet.window_draws_for(3)[0] == (224, 160)
    val = ValidationAugmentation(Namespace(width=128, height=96, train_tiles="2x2", tile_overlap=32))
    state = torch.get_rng_state()
    assert val.window_draws_for(3) is None and torch.equal(torch.get_rng_state(), state)


def test_window_annotation_rule_on_hand_cases():
    """resize to the canvas, then the shift by the origin under affine_annotation's rule: a point is inside iff 0 <= x' + 0.5 < w."""
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    from structuredetector_amd.utils.misc import affine_annotation
    (win, hin), (Wc, Hc), (w, h), (x0, y0) = (448, 320), (224, 160), (128, 96), (40, 20)     # canvas = source / 2: exact arithmetic
    mk = lambda name, a, parts: Object(name, Keypoint("stem", *a), [Keypoint(f"p{j}", *p) for j, p in enumerate(parts)])
    ann = ImageAnnotation("a.png", [
        mk("inside", (80.0, 40.0), [(100.0, 60.0)]),              # canvas (40, 20) -> window (0, 0): kept, at the very corner
        mk("just_out_left", (78.0, 100.0), [(200.0, 100.0)]),     # canvas x 39 -> window x -1, centre -0.5 < 0: the object leaves with its anchor
        mk("just_in_right", (334.0, 100.0), [(336.0, 100.0), (100.0, 230.0), (100.0, 232.0)]),
        mk("below", (100.0, 232.0), []),
    ])
    ann.resize((win, hin), (Wc, Hc))
    affine_annotation(ann, [1, 0, -x0, 0, 1, -y0], (w, h))
    rows = {o.name: ((o.x, o.y), [(p.kind, p.x, p.y) for p in o.parts]) for o in ann.objects}
    assert set(rows) == {"inside", "just_in_right"}
    assert rows["inside"] == ((0.0, 0.0), [("p0", 10.0, 10.0)])
    # anchor at canvas x 167 -> window x 127 (centre 127.5 < 128: kept); the part at canvas x 168 -> 128 is outside; the part at canvas
    # y 115 -> window y 95 is kept, the one at y 116 -> 96 is dropped
    assert rows["just_in_right"] == ((127.0, 30.0), [("p1", 10.0, 95.0)])


def test_c_abi_rejects_bad_arguments_before_any_launch():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    Bn, Hin, Win, Hc, Wc, Hout, Wout = 2, 16, 30000, 12, 96, 8, 64
    need = lib.sd_preprocess_window_workspace_bytes(Bn, Hin, Hout, Wout)
    assert need >= Bn * Hin * Wout * 3 + 2 * Bn * Hout * Wout * 3 + Bn * 8
    m3, s3, fill = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25), (C.c_ubyte * 3)(*FILL)
    P = 4096                                                                   # never dereferenced: no call below reaches a launch
    for fn, name, is_list in ((lib.sd_preprocess_images_window, b"sd_preprocess_images_window", False),
                              (lib.sd_preprocess_images_list_window, b"sd_preprocess_images_list_window", True)):
        def call(window=P, rows=Hin, cols=100, order=None, factors=None, affine=None, geom=None, mats=None, fill3=fill, ws=need, hout=Hout):
            return fn(P, Bn, Hin, Win, Hc, Wc, hout, Wout, P, P, 3, P, P, 3, window, rows, cols, None, order, factors, affine, geom, mats, fill3,
                      m3, s3, P, P, ws, 0)
        cases = [("a jitter table alone", dict(order=P), -1), ("jitter factors alone", dict(factors=P), -1), ("a null window table", dict(window=None), -1),
                 ("mosaic geometry alone", dict(geom=P), -1), ("a warp without a fill colour", dict(affine=P, fill3=None), -1),
                 ("a window taller than the canvas", dict(hout=Hc + 1), -1), ("max_rows over the source", dict(rows=Hin + 1), -1),
                 ("max_cols of zero", dict(cols=0), -1), ("a workspace one byte short", dict(ws=need - 1), -2)]
        if is_list:
            cases.append(("max_cols over the LDS limit", dict(cols=21835), -1))
        for what, kw, code in cases:
            lib.sd_set_option(b"no_such_option", 1)                            # leaves another message behind
            assert call(**kw) == code, f"{name.decode()}: {what}"
            assert lib.sd_last_error() and name in lib.sd_last_error(), f"{name.decode()}: {what}: {lib.sd_last_error()}"
    assert b"LDS" in lib.sd_last_error() and b"21834" in lib.sd_last_error()
