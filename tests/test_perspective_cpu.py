"""Random perspective augmentation (`--aug_perspective`), the parts that need no GPU: tests/perspective_ref.py against Pillow itself byte
for byte, the coefficient helpers, the annotations, the flag and its draws, and the argument checks of the C entry points."""
import ctypes as C
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.affine_ref import affine_bilinear, blob_image
from tests.perspective_ref import (DISTORTIONS, FILL, IDENTITY, SEEDS, SIZES, affine_rows, frame_quad, hand_made, image, perspective_bilinear,
                                   pil_perspective, policy_coeffs, policy_quad, positions)

INSIDE_FLOOR = 0.3              # the smallest share of sampled pixels a policy case with D <= 0.5 may have: the comparison is not of fill alone


def _equal(img, a, what):
    got, inside = perspective_bilinear(img, a)
    want = pil_perspective(img, a)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {bad.sum()} pixels differ, first at {np.argwhere(bad)[0].tolist()}"
    return got, inside


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_restatement_equals_pillow_on_policy_quads(size):
    H, W = size
    img = image(H, W)
    for D in DISTORTIONS:
        for seed in SEEDS:
            inverse, _ = policy_coeffs(W, H, D, seed)
            _, inside = _equal(img, inverse, f"{size} D {D} seed {seed}")
            if D <= 0.5:                                                                # (D = 0.9 is compared, not counted)
                assert inside.mean() >= INSIDE_FLOOR, f"{size} D {D} seed {seed}: only {inside.mean():.3f} of the pixels are sampled"


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_identity_and_pure_affine_rows_equal_pillow_and_the_affine_restatement(size):
    H, W = size
    img = image(H, W, 1)
    got, inside = _equal(img, IDENTITY, "identity")
    assert np.array_equal(got, img) and inside.all()                                    # a copy
    for row in affine_rows(W, H):
        got, inside = _equal(img, row, f"{size} affine {row[:6]}")
        want, want_inside = affine_bilinear(img, row[:6])
        assert np.array_equal(got, want) and np.array_equal(inside, want_inside)        # x / 1.0 is exact


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_hand_made_denominators_equal_pillow(size):
    H, W = size
    img = image(H, W, 2)
    rows = hand_made(W, H)
    for name, a in rows.items():
        xin, yin, den = positions(H, W, a)
        assert not (np.isnan(xin) | np.isnan(yin)).any(), name                          # Pillow is undefined at NaN: no case has one
        got, inside = _equal(img, a, f"{size} {name}")
        if name == "zero":
            assert den[0, 1] == 0.0 and np.isinf(xin[0, 1]) and np.isinf(yin[0, 1])     # exactly 0 at the pixel centre (1.5, 0.5)
            assert not inside[0, 1] and tuple(got[0, 1]) == FILL
    _, _, den = positions(96, 128, rows["sign"])
    assert (den > 0).any() and (den < 0).any()                                          # the sign changes inside the frame
    _, _, den = positions(96, 128, rows["behind"])
    _, inside = perspective_bilinear(image(96, 128, 2), rows["behind"])
    assert (den > 0).any() and inside[den < 0].mean() > 0.5                             # a negative denominator samples the source, as in Pillow


def _apply(a, x, y):
    den = a[6] * x + a[7] * y + 1.0
    return (a[0] * x + a[1] * y + a[2]) / den, (a[3] * x + a[4] * y + a[5]) / den


def test_perspective_coeffs_forward_and_inverse_compose_to_the_identity():
    from structuredetector_amd.data import perspective_coeffs
    W, H = 64, 48
    xc, yc = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    for D in DISTORTIONS:
        for seed in SEEDS:
            quad = policy_quad(W, H, D, seed)
            inverse, forward = perspective_coeffs(frame_quad(W, H), quad), perspective_coeffs(quad, frame_quad(W, H))
            for (qx, qy), (fx, fy) in zip(quad, frame_quad(W, H)):                      # the corners go where they were asked to
                assert np.allclose(_apply(inverse, qx, qy), (fx, fy), atol=1e-9) and np.allclose(_apply(forward, fx, fy), (qx, qy), atol=1e-9)
            bx, by = _apply(inverse, *_apply(forward, xc, yc))
            assert np.abs(bx - xc).max() <= 1e-9 and np.abs(by - yc).max() <= 1e-9, (D, seed)
    assert np.allclose(perspective_coeffs(frame_quad(W, H), frame_quad(W, H)), IDENTITY, atol=1e-15)


def test_compose_affine_perspective():
    from structuredetector_amd.data import affine_inverse_matrix, compose_affine_perspective
    W, H = 64, 48
    affine = affine_inverse_matrix((W, H), 17.3, 1.1, (3.25, -4.5))
    persp, _ = policy_coeffs(W, H, 0.5, 3)
    assert compose_affine_perspective(affine, IDENTITY) == [*affine, 0.0, 0.0]          # exactly
    assert compose_affine_perspective([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], persp) == list(persp)
    both = compose_affine_perspective(affine, persp)
    assert both[6:] == list(persp[6:])                                                  # the last row is P's: nothing is renormalised
    for x, y in ((0.5, 0.5), (31.5, 20.5), (63.5, 47.5)):
        px, py = _apply(persp, x, y)
        want = (affine[0] * px + affine[1] * py + affine[2], affine[3] * px + affine[4] * py + affine[5])
        assert np.allclose(_apply(both, x, y), want, atol=1e-9)


# ---- annotations -------------------------------------------------------------------------------------------------------------------
def _annotation(objects):
    from structuredetector_amd.utils import Box, ImageAnnotation, Keypoint, Object
    return ImageAnnotation("a.png", [Object(label, Keypoint("stem", *anchor), [Keypoint("leaf", *p) for p in parts],
                                            None if box is None else Box(*box)) for label, anchor, parts, box in objects])


def test_perspective_annotation_keeps_what_the_image_shows_and_drops_the_rest():
    from structuredetector_amd.utils import perspective_annotation
    W, H = 64, 48
    rng = np.random.default_rng(3)
    for D, seed in ((0.3, 0), (0.5, 1), (0.9, 2), (0.9, 4)):
        inverse, forward = policy_coeffs(W, H, D, seed)
        _, inside = perspective_bilinear(image(H, W), inverse)
        points = [(float(x), float(y)) for x, y in zip(rng.uniform(-0.49, W - 0.51, 60), rng.uniform(-0.49, H - 0.51, 60))]
        points += [(0.0, 0.0), (W - 1.0, 0.0), (W - 1.0, H - 1.0), (0.0, H - 1.0)]     # the corner pixels move inwards
        ann = perspective_annotation(_annotation([("bean", p, [], None) for p in points]), forward, (W, H))
        kept = [(o.x, o.y) for o in ann.objects]
        assert 0 < len(kept) <= len(points)
        moved, interior = {}, 0
        for x, y in points:
            den = forward[6] * (x + 0.5) + forward[7] * (y + 0.5) + 1.0
            fx, fy = _apply(forward, x + 0.5, y + 0.5)
            moved[(x, y)] = (fx - 0.5, fy - 0.5, den)
        want = [(mx, my) for mx, my, den in moved.values() if den > 0 and 0 <= mx + 0.5 < W and 0 <= my + 0.5 < H]
        assert kept == want                                                             # in order; the others were dropped
        for (x, y), (mx, my, den) in moved.items():
            if (mx, my) in kept:
                bx, by = _apply(inverse, mx + 0.5, my + 0.5)
                assert abs(bx - (x + 0.5)) <= 1e-6 and abs(by - (y + 0.5)) <= 1e-6      # the image shows source point p at p'
                # the landing pixel is sampled, not filled.  Its centre lies up to half a pixel from p' + 0.5, so this is asserted for the
                # points at least 4 source pixels from the border at D <= 0.5, where a side keeps at least half its length
                if D <= 0.5 and 4 <= x <= W - 5 and 4 <= y <= H - 5:
                    assert inside[int(math.floor(my + 0.5)), int(math.floor(mx + 0.5))], (D, seed, x, y)
                    interior += 1
            else:
                px, py = math.floor(mx + 0.5), math.floor(my + 0.5)
                assert den <= 0 or not (0 <= px < W and 0 <= py < H)
        assert D > 0.5 or interior >= 20


def test_a_point_behind_the_horizon_is_dropped_even_where_it_would_land_inside():
    from structuredetector_amd.utils import perspective_annotation
    W, H = 64, 48
    forward = [-1.0, 0.0, 0.0, 0.0, -1.0, 0.0, -0.1, 0.0]                               # den = 1 - 0.1 (x + 0.5): negative from x = 10 on
    x, y = 30.0, 20.0
    den = forward[6] * (x + 0.5) + 1.0
    fx, fy = _apply(forward, x + 0.5, y + 0.5)
    assert den < 0 and 0 <= fx < W and 0 <= fy < H                                      # it would land inside the frame
    ann = perspective_annotation(_annotation([("bean", (x, y), [], None)]), forward, (W, H))
    assert ann.objects == []
    flipped = [-v for v in forward[:6]] + [0.1, 0.0]                                    # the same landing point with a positive denominator stays
    ann = perspective_annotation(_annotation([("bean", (x, y), [], None)]), flipped, (W, H))
    assert len(ann.objects) == 1


def test_an_object_leaves_with_its_anchor_a_failing_part_alone_and_a_box_becomes_its_hull():
    from structuredetector_amd.data import perspective_coeffs
    from structuredetector_amd.utils import perspective_annotation
    W, H = 64, 48
    quad = [(20.0, 10.0), (60.0, 4.0), (62.0, 44.0), (16.0, 40.0)]                      # the frame shrinks towards the right: the left edge moves in
    forward = perspective_coeffs(quad, frame_quad(W, H))
    inverse = perspective_coeffs(frame_quad(W, H), quad)
    # an affine shift by -60 first, with no drop in between: the image is resampled once, so what the shift moves out of the frame and the
    # perspective brings back in is shown and kept; only the final position decides
    shift = [1.0, 0.0, -60.0, 0.0, 1.0, 0.0]
    final = lambda x, y: tuple(v - 0.5 for v in _apply(forward, x + 0.5 - 60.0, y + 0.5))
    assert final(5.0, 20.0)[0] + 0.5 < 0 and final(10.0, 20.0)[0] + 0.5 < 0             # the first anchor and one part end left of the frame
    assert all(0 <= final(x, y)[0] + 0.5 < W and 0 <= final(x, y)[1] + 0.5 < H for x, y in ((40.0, 20.0), (50.0, 20.0), (45.0, 25.0)))
    assert 50.5 - 60.0 < 0                                                              # the kept anchor was outside after the shift alone
    ann = _annotation([("gone", (5.0, 20.0), [(40.0, 20.0)], None),                    # anchor out: the object goes, with its inside part
                       ("stays", (50.0, 20.0), [(45.0, 25.0), (10.0, 20.0)], (40.0, 10.0, 60.0, 30.0))])
    ann = perspective_annotation(ann, forward, (W, H), affine_forward=shift)
    assert [o.name for o in ann.objects] == ["stays"]
    obj = ann.objects[0]
    assert len(obj.parts) == 1                                                          # (10, 20) left, (45, 25) stayed
    assert (obj.x, obj.y) == final(50.0, 20.0) and (obj.parts[0].x, obj.parts[0].y) == final(45.0, 25.0)
    corners = [final(x, y) for x in (40.0, 60.0) for y in (10.0, 30.0)]
    xs, ys = [c[0] for c in corners], [c[1] for c in corners]
    b = obj.box
    assert (b.x_min, b.x_max, b.y_min, b.y_max) == (min(xs), max(xs), min(ys), max(ys))
    assert len({round(v, 9) for v in xs}) == 4                                          # a true quadrilateral: the hull is larger than any edge
    # the identity homography with an affine matrix is affine_annotation
    from structuredetector_amd.data import affine_forward_matrix
    from structuredetector_amd.utils import affine_annotation
    f6 = affine_forward_matrix((W, H), 17.3, 1.1, (3.25, -4.5))
    objects = [("a", (30.0, 20.0), [(33.0, 22.0), (1.0, 1.0)], (25.0, 15.0, 35.0, 25.0)), ("b", (63.0, 0.0), [], None)]
    got = perspective_annotation(_annotation(objects), list(IDENTITY), (W, H), affine_forward=f6)
    want = affine_annotation(_annotation(objects), f6, (W, H))
    rows = lambda a: [(o.name, o.x, o.y, [(p.x, p.y) for p in o.parts], o.box and (o.box.x_min, o.box.x_max, o.box.y_min, o.box.y_max)) for o in a.objects]
    assert rows(got) == rows(want) and len(rows(got)) >= 1
    del inverse


def test_affine_then_perspective_annotations_follow_the_composite_image():
    """A blob at a keypoint, warped ONCE by the composed coefficients, is found again at the pixel perspective_annotation moves the keypoint
    to with the affine forward matrix first."""
    from structuredetector_amd.data import affine_forward_matrix, affine_inverse_matrix, compose_affine_perspective
    from structuredetector_amd.utils import perspective_annotation
    H, W = 96, 128
    checked = 0
    for (angle, scale, tx, ty), D, seed in (((17.3, 1.1, 3.25, -4.5), 0.3, 0), ((-45, 0.75, 0, 0), 0.5, 1), ((5, 0.9, 10.5, 10.5), 0.5, 2),
                                            ((0, 1, 0, 0), 0.5, 3)):
        inverse, forward = policy_coeffs(W, H, D, seed)
        row = compose_affine_perspective(affine_inverse_matrix((W, H), angle, scale, (tx, ty)), inverse)
        for kx, ky in ((64, 48), (40, 30), (90, 60)):
            warped = pil_perspective(blob_image(H, W, [(kx, ky)]), row, fill=(0, 0, 0))
            ann = perspective_annotation(_annotation([("bean", (float(kx), float(ky)), [], None)]), forward, (W, H),
                                         affine_forward=affine_forward_matrix((W, H), angle, scale, (tx, ty)))
            if not ann.objects:
                continue
            px, py = int(math.floor(ann.objects[0].x + 0.5)), int(math.floor(ann.objects[0].y + 0.5))
            assert warped[py, px, 0] >= 128, (angle, D, seed, kx, ky, warped[py, px].tolist())
            ys, xs = np.nonzero(warped[..., 0] >= 128)
            assert abs(xs.mean() - ann.objects[0].x) <= 1.0 and abs(ys.mean() - ann.objects[0].y) <= 1.0      # and it is the blob's centre
            checked += 1
    assert checked >= 9


# ---- the flag and its draws --------------------------------------------------------------------------------------------------------
def test_flag_parses_defaults_to_off_and_is_range_checked():
    from structuredetector_amd.utils.args import Arguments, check_aug_perspective
    parser = Arguments().parser
    assert parser.parse_args([]).aug_perspective == 0.0
    assert parser.parse_args(["--aug_perspective", "0.3"]).aug_perspective == 0.3
    text = " ".join(parser.format_help().split())
    assert "--aug_perspective D" in text and "PERSPECTIVE" in text
    for bad in ("-0.1", "0.95"):
        with pytest.raises(AssertionError, match="aug_perspective"):
            Arguments().parse(["--aug_perspective", bad])
    assert check_aug_perspective(parser.parse_args([])) == 0.0
    assert check_aug_perspective(Namespace()) == 0.0                                    # a namespace from before the flag
    assert check_aug_perspective(parser.parse_args(["--aug_perspective", "0.9"])) == 0.9
    assert check_aug_perspective(parser.parse_args(["--synthetic", "8"])) == 0.0        # off: --synthetic is fine
    for bad in (-0.1, 0.91, 1.0, float("nan")):
        with pytest.raises(ValueError, match="aug_perspective"):
            check_aug_perspective(Namespace(aug_perspective=bad))
    with pytest.raises(ValueError, match="'aug_perspective' warps source images: it needs --train_dir, not --synthetic"):
        check_aug_perspective(parser.parse_args(["--aug_perspective", "0.3", "--synthetic", "8"]))
    from structuredetector_amd.model.trainer import Trainer
    with pytest.raises(ValueError, match="needs --train_dir, not --synthetic"):         # `train` checks before it builds anything (no GPU is touched)
        Trainer(parser.parse_args(["--aug_perspective", "0.3", "--synthetic", "8"]))


_COMMON = dict(width=128, height=96, no_augmentation=False, aug_rotate=10.0, aug_mosaic=0.5, aug_transpose=0.0, aug_blur=2.0, train_tiles="",
               device="cpu")


def _all_draws(aug, n, groups):
    """The draws of `__call__`, in its order."""
    return (aug.draws_for(n), aug.affine_draws_for(n), aug.mosaic_draws_for(n, groups), aug.window_draws_for(n), aug.transpose_draws_for(n),
            aug.blur_draws_for(n), aug.perspective_draws_for(n))


def test_no_draw_when_off_and_one_draw_when_on():
    from structuredetector_amd.data import TrainAugmentation, ValidationAugmentation
    n, groups = 6, [[0, 1, 2], [3, 4, 5]]
    torch.manual_seed(3)
    _all_draws(TrainAugmentation(Namespace(**_COMMON)), n, groups)                      # a namespace without the attribute
    without = torch.get_rng_state()
    for extra in (dict(aug_perspective=0.0), dict(aug_perspective=0)):
        aug = TrainAugmentation(Namespace(**{**_COMMON, **extra}))
        torch.manual_seed(3)
        assert _all_draws(aug, n, groups)[-1] is None
        assert torch.equal(torch.get_rng_state(), without), extra                       # the generator is where it was without the flag
    aug = TrainAugmentation(Namespace(**{**_COMMON, "aug_perspective": 0.5, "no_augmentation": True}))
    before = torch.get_rng_state()
    assert aug.perspective_draws_for(n) is None and torch.equal(torch.get_rng_state(), before)
    val = ValidationAugmentation(Namespace(width=128, height=96, aug_perspective=0.5))
    assert val.perspective_draws_for(n) is None and torch.equal(torch.get_rng_state(), before)
    aug = TrainAugmentation(Namespace(**_COMMON, aug_perspective=0.3))
    torch.manual_seed(3)
    quads = aug.perspective_draws_for(64)
    torch.manual_seed(3)
    u = torch.rand(64, 9, dtype=torch.float64).tolist()                                 # ONE draw: rand(n, 9) in float64
    assert torch.equal(torch.get_rng_state(), _state_after(aug, 64))
    W, H, D = 128, 96, 0.3                                                              # (no power of two: the products as stated, left to right)
    for q, r in zip(quads, u):
        if r[0] < 0.5:
            assert q == [(r[1] * D * W / 2, r[2] * D * H / 2), (W - r[3] * D * W / 2, r[4] * D * H / 2),
                         (W - r[5] * D * W / 2, H - r[6] * D * H / 2), (r[7] * D * W / 2, H - r[8] * D * H / 2)]
        else:
            assert q is None
    assert any(q is None for q in quads) and any(q is not None for q in quads)
    aug.size = (96, 64)                                                                 # the insets follow the current multi-scale size
    torch.manual_seed(3)
    small = aug.perspective_draws_for(64)
    k = next(i for i, q in enumerate(quads) if q is not None)
    assert small[k][2] == (96 - u[k][5] * D * 96 / 2, 64 - u[k][6] * D * 64 / 2)


def _state_after(aug, n):
    torch.manual_seed(3)
    aug.perspective_draws_for(n)
    return torch.get_rng_state()


def test_earlier_draws_of_a_batch_do_not_depend_on_the_flag():
    """The perspective draw comes last: flips, jitter, warp, mosaic, window, transpose and blur draws are the same with the flag on and off."""
    from structuredetector_amd.data import TrainAugmentation
    common = {**_COMMON, "width": 128, "height": 128, "aug_transpose": 0.5, "train_tiles": "2x2", "tile_overlap": 32}
    seen = []
    for d in (0.0, 0.5):
        aug = TrainAugmentation(Namespace(**common, aug_perspective=d))
        torch.manual_seed(11)
        draws = _all_draws(aug, 8, [[0, 1, 2, 3], [4, 5, 6, 7]])
        assert all(x is not None for x in draws[:-1]) and (draws[-1] is None) == (d == 0.0)
        seen.append(draws[:-1])
    assert seen[0] == seen[1]


# ---- the library -------------------------------------------------------------------------------------------------------------------
NAMES = ("sd_perspective_u8", "sd_preprocess_images_persp", "sd_preprocess_images_list_persp")


def test_library_exports_the_perspective_symbols():
    from pathlib import Path
    from structuredetector_amd import _lib as L
    handle = L.lib()
    assert set(NAMES) <= set(L.declared_symbols())
    assert all(hasattr(handle, n) for n in NAMES)
    header = (Path(__file__).resolve().parents[1] / "include" / "sdnet_hip.h").read_text()
    assert all(f"int {n}(" in header for n in NAMES)
    from structuredetector_amd import data, utils
    assert all(hasattr(data, n) for n in ("perspective_coeffs", "compose_affine_perspective", "perspective_images"))
    assert hasattr(utils, "perspective_annotation")


def test_sd_perspective_u8_rejects_bad_arguments_without_touching_the_gpu():
    """Every bad call returns before a launch (the pointers are never dereferenced) and sd_last_error() names the function."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    fill = (C.c_ubyte * 3)(*FILL)

    def call(src=4096, dst=1 << 20, B=2, H=5, W=7, coeffs=2 << 20, fill3=fill):
        return lib.sd_perspective_u8(src, dst, B, H, W, coeffs, fill3, 0)

    n = 2 * 5 * 7 * 3
    for kw, text in [(dict(src=0), "null"), (dict(dst=0), "null"), (dict(coeffs=0), "null"), (dict(fill3=None), "null"),
                     (dict(dst=4096), "in place"), (dict(dst=4096 + n - 1), "overlap"), (dict(dst=4096 - n + 1), "overlap"),
                     (dict(B=0), "bad shape"), (dict(H=0), "bad shape"), (dict(W=-1), "bad shape"), (dict(B=65536), "too large")]:
        lib.sd_set_option(b"no_such_option", 1)                                         # leaves another message behind
        assert call(**kw) == -1, kw                                                     # SD_ERR_INVALID
        msg = lib.sd_last_error().decode()
        assert "sd_perspective_u8" in msg and text in msg, (kw, msg)


def test_chain_forms_reject_persp_with_affine_and_a_missing_fill_without_touching_the_gpu():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    Bn, Hin, Win, Hout, Wout = 2, 8, 8, 4, 4
    need = lib.sd_preprocess_blur_workspace_bytes(0, Bn, Hin, Win, 0, Hout, Wout, 0)
    m3, s3, fill = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25), (C.c_ubyte * 3)(*FILL)
    P = 4096                                                                            # never dereferenced: no call below reaches a launch
    for name in NAMES[1:]:
        fn = getattr(lib, name)

        def call(affine=None, persp=P, fill3=fill, ws=need, geometry=0):
            return fn(P, geometry, Bn, Hin, Win, 0, 0, Hout, Wout, 0, 0, P, P, 3, P, P, 3, None, None, None, None, affine, persp, None, None, None,
                      fill3, m3, s3, P, P, ws, 0)
        for what, kw, code, text in (("persp with affine", dict(affine=P), -1, "do not combine"), ("no fill colour", dict(fill3=None), -1, "fill"),
                                     ("unknown geometry", dict(geometry=7), -1, "geometry"),
                                     ("workspace one byte short", dict(ws=need - 1), -2, "workspace"),
                                     ("null persp is the blur form: its geometry check", dict(persp=None, geometry=7), -1, "geometry")):
            lib.sd_set_option(b"no_such_option", 1)
            assert call(**kw) == code, f"{name}: {what}"
            msg = lib.sd_last_error().decode()
            assert text in msg and (name in msg or kw.get("persp", P) is None), f"{name}: {what}: {msg}"
