"""Random affine augmentation (`--aug_rotate / --aug_scale / --aug_translate`), the parts that need no GPU: the numpy restatement of
Pillow's affine + bilinear transform against Pillow itself, the matrix helpers, the annotation transform and its drop rule, the image /
annotation consistency, the random draws and the flags."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.affine_ref import FILL, PARAMS, SIZES, affine_bilinear, blob_image, pil_affine


def _annotation(objects):
    from structuredetector_amd.utils import Box, ImageAnnotation, Keypoint, Object
    return ImageAnnotation("a.png", [Object(name, Keypoint("stem", *anchor), [Keypoint("leaf", *p) for p in parts], Box(*box) if box else None)
                                     for name, anchor, parts, box in objects])


def test_restatement_equals_pillow_bitwise_on_28_cases():
    """4 sizes x 7 parameter sets; no case is trivially all fill or all copy: every case keeps >= 40 % of its output inside the source
    and at least half of the cases have >= 4 % fill."""
    from structuredetector_amd.data.augment import _FILL, affine_inverse_matrix
    assert _FILL == FILL == (124, 116, 104)
    rng = np.random.default_rng(2024)
    fills, pixels = [], 0
    for H, W in SIZES:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for angle, scale, tx, ty in PARAMS:
            m = affine_inverse_matrix((W, H), angle, scale, (tx, ty))
            got, inside = affine_bilinear(img, m)
            want = pil_affine(img, m)
            assert np.array_equal(got, want), f"{(H, W)} {(angle, scale, tx, ty)}: {(got != want).any(-1).sum()} pixels differ"
            share = inside.mean()
            assert share >= 0.40, f"{(H, W)} {(angle, scale, tx, ty)}: only {share:.2%} inside"
            fills.append(1 - share)
            pixels += H * W
    assert len(fills) == 28 and pixels == 7 * sum(h * w for h, w in SIZES)
    assert sum(f >= 0.04 for f in fills) >= 14, sorted(fills)


def test_matrix_helpers():
    from structuredetector_amd.data.augment import affine_forward_matrix, affine_inverse_matrix
    assert affine_inverse_matrix((128, 96), 0, 1, (0, 0)) == [1, 0, 0, 0, 1, 0]
    assert affine_inverse_matrix((47, 33), 0.0, 1.0, (0.0, 0.0)) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    for (H, W) in SIZES:
        for angle, scale, tx, ty in PARAMS:
            i = affine_inverse_matrix((W, H), angle, scale, (tx, ty))
            f = affine_forward_matrix((W, H), angle, scale, (tx, ty))
            I3 = np.array([i[:3], i[3:], [0, 0, 1]], np.float64)
            F3 = np.array([f[:3], f[3:], [0, 0, 1]], np.float64)
            assert np.abs(F3 @ I3 - np.eye(3)).max() <= 1e-12 and np.abs(I3 @ F3 - np.eye(3)).max() <= 1e-12


def test_half_turn_equals_both_flips():
    from structuredetector_amd.data.augment import affine_forward_matrix
    from structuredetector_amd.utils import affine_annotation, hflip_annotation, vflip_annotation
    size = (128, 96)
    objects = [("bean", (10.0, 20.5), [(100.25, 90.0), (0.0, 0.0)], (5.0, 10.0, 30.0, 40.0)), ("maize", (127.0, 95.0), [(64.0, 48.0)], None)]
    a = affine_annotation(_annotation(objects), affine_forward_matrix(size, 180, 1, (0, 0)), size)
    b = vflip_annotation(hflip_annotation(_annotation(objects), size), size)
    assert len(a.objects) == len(b.objects) == 2
    for oa, ob in zip(a.objects, b.objects):
        assert abs(oa.x - ob.x) <= 1e-9 and abs(oa.y - ob.y) <= 1e-9 and len(oa.parts) == len(ob.parts)
        for pa, pb in zip(oa.parts, ob.parts):
            assert abs(pa.x - pb.x) <= 1e-9 and abs(pa.y - pb.y) <= 1e-9
        if ob.box is not None:
            for k in ("x_min", "x_max", "y_min", "y_max"):
                assert abs(getattr(oa.box, k) - getattr(ob.box, k)) <= 1e-9
    assert isinstance(a.objects[0].x, float)


def test_drop_rule_and_box_hull():
    """Shift by (+40, 0) on a 128 x 96 frame, then a quarter turn for the hull."""
    from structuredetector_amd.data.augment import affine_forward_matrix
    from structuredetector_amd.utils import affine_annotation
    size = (128, 96)
    ann = _annotation([("gone", (100.0, 50.0), [(20.0, 20.0), (30.0, 30.0)], None),                # anchor x 140: out, with its parts
                       ("kept", (60.0, 40.0), [(10.0, 10.0), (90.0, 45.0), (87.5, 95.0)], None),    # part 2 -> x 130: out; part 3 -> x 127.5: out
                       ("edge", (87.0, 0.0), [(87.49, 95.49)], None)])                             # x' + 0.5 = 127.5 / 127.99 < 128: in
    affine_annotation(ann, affine_forward_matrix(size, 0, 1, (40, 0)), size)
    assert [o.name for o in ann.objects] == ["kept", "edge"]
    kept, edge = ann.objects
    assert (kept.x, kept.y) == (100.0, 40.0) and [(p.x, p.y) for p in kept.parts] == [(50.0, 10.0)]
    assert (edge.x, edge.y) == (127.0, 0.0) and len(edge.parts) == 1 and abs(edge.parts[0].x - 127.49) < 1e-9
    # the drop test is Pillow's inside test, at the left edge too: x' + 0.5 = -0.01 is out, 0.0 is in
    ann = _annotation([("in", (39.5, 5.0), [], None), ("out", (39.49, 5.0), [], None)])
    affine_annotation(ann, affine_forward_matrix(size, 0, 1, (-40, 0)), size)
    assert [o.name for o in ann.objects] == ["in"] and ann.objects[0].x == -0.5
    # a box becomes the hull of its four corners: 30 degrees about the centre
    f = affine_forward_matrix(size, 30, 1, (0, 0))
    ann = _annotation([("box", (64.0, 48.0), [], (54.0, 43.0, 74.0, 53.0))])
    affine_annotation(ann, f, size)
    corners = [(f[0] * (x + 0.5) + f[1] * (y + 0.5) + f[2] - 0.5, f[3] * (x + 0.5) + f[4] * (y + 0.5) + f[5] - 0.5)
               for x in (54.0, 74.0) for y in (43.0, 53.0)]
    b = ann.objects[0].box
    assert (b.x_min, b.x_max) == (min(c[0] for c in corners), max(c[0] for c in corners))
    assert (b.y_min, b.y_max) == (min(c[1] for c in corners), max(c[1] for c in corners))
    assert b.x_max - b.x_min > 20.0 and b.y_max - b.y_min > 10.0                    # wider and taller than the 20 x 10 box it was
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    assert abs((b.x_max - b.x_min) - (20 * c + 10 * s)) < 1e-9 and abs((b.y_max - b.y_min) - (20 * s + 10 * c)) < 1e-9


def test_image_and_annotation_move_together():
    """A 3 x 3 white blob on a keypoint, warped by the restatement: the intensity-weighted centroid of the output lies within 0.75 px of
    where affine_annotation puts the keypoint."""
    from structuredetector_amd.data.augment import affine_forward_matrix, affine_inverse_matrix
    from structuredetector_amd.utils import affine_annotation
    H, W = 96, 128
    angle, scale, tx, ty = 17.3, 1.1, 3.25, -4.5
    for kx, ky in ((40, 30), (90, 60), (64, 48)):
        out, _ = affine_bilinear(blob_image(H, W, [(kx, ky)]), affine_inverse_matrix((W, H), angle, scale, (tx, ty)), fill=(0, 0, 0))
        wgt = out[..., 0].astype(np.float64)
        assert wgt.sum() > 0
        cx = (wgt * np.arange(W)[None, :]).sum() / wgt.sum()
        cy = (wgt * np.arange(H)[:, None]).sum() / wgt.sum()
        ann = affine_annotation(_annotation([("bean", (float(kx), float(ky)), [], None)]), affine_forward_matrix((W, H), angle, scale, (tx, ty)), (W, H))
        assert math.hypot(cx - ann.objects[0].x, cy - ann.objects[0].y) <= 0.75, (cx, cy, ann.objects[0])


def test_draws_off_consume_nothing_and_on_stay_in_range():
    from structuredetector_amd.data import TrainAugmentation, ValidationAugmentation
    off = Namespace(width=128, height=96, no_augmentation=False, device=None, aug_rotate=0.0, aug_scale=0.0, aug_translate=0.0)
    torch.manual_seed(7)
    before = torch.get_rng_state()
    assert TrainAugmentation(off).affine_draws_for(64) is None
    assert TrainAugmentation(Namespace(width=128, height=96, no_augmentation=False, device=None)).affine_draws_for(64) is None     # flags absent
    on = Namespace(width=128, height=96, no_augmentation=False, device=None, aug_rotate=30.0, aug_scale=0.2, aug_translate=0.1)
    assert ValidationAugmentation(on).affine_draws_for(64) is None
    quiet = Namespace(**{**vars(on), "no_augmentation": True})
    assert TrainAugmentation(quiet).affine_draws_for(64) is None
    assert torch.equal(torch.get_rng_state(), before)
    # off: draws_for consumes what it always did (one rand(n, 8) in float64 + one randn(n, 2))
    flips, jitter = TrainAugmentation(off).draws_for(5)
    mid = torch.get_rng_state()
    torch.set_rng_state(before)
    torch.rand(5, 8, dtype=torch.float64); torch.randn(5, 2)
    assert torch.equal(torch.get_rng_state(), mid) and len(flips) == 5 and len(jitter[0]) == 5
    aug = TrainAugmentation(on)
    draws = aug.affine_draws_for(4096)
    assert not torch.equal(torch.get_rng_state(), mid) and len(draws) == 4096
    d = np.asarray(draws)
    assert (np.abs(d[:, 0]) <= 30.0).all() and (d[:, 1] >= 0.8).all() and (d[:, 1] <= 1.2).all()
    assert (np.abs(d[:, 2]) <= 0.1 * 128).all() and (np.abs(d[:, 3]) <= 0.1 * 96).all()
    assert d[:, 0].min() < -25 and d[:, 0].max() > 25 and d[:, 1].min() < 0.83 and d[:, 1].max() > 1.17          # the ranges are used
    assert d[:, 2].min() < -11 and d[:, 2].max() > 11 and d[:, 3].min() < -8.5 and d[:, 3].max() > 8.5
    aug.size = (160, 64)                                                     # the shift follows the multi-scale size
    d = np.asarray(aug.affine_draws_for(4096))
    assert (np.abs(d[:, 2]) <= 16.0).all() and d[:, 2].max() > 14.5 and (np.abs(d[:, 3]) <= 6.4).all()
    only = TrainAugmentation(Namespace(**{**vars(off), "aug_rotate": 10.0}))
    d = np.asarray(only.affine_draws_for(256))
    assert (d[:, 1] == 1.0).all() and (d[:, 2] == 0.0).all() and (d[:, 3] == 0.0).all() and np.abs(d[:, 0]).max() > 5


def test_flags_parse_default_off_and_validate():
    from structuredetector_amd.utils.args import Arguments, finalize
    parser = Arguments().parser
    ns = parser.parse_args([])
    assert (ns.aug_rotate, ns.aug_scale, ns.aug_translate) == (0.0, 0.0, 0.0)
    ns = parser.parse_args(["--aug_rotate", "30", "--aug_scale", "0.2", "--aug_translate", "0.1"])
    assert (ns.aug_rotate, ns.aug_scale, ns.aug_translate) == (30.0, 0.2, 0.1)
    text = " ".join(parser.format_help().split())
    assert "--aug_rotate DEG" in text and "--aug_scale S" in text and "--aug_translate T" in text
    for bad in (["--aug_rotate", "-1"], ["--aug_rotate", "180.5"], ["--aug_scale", "1"], ["--aug_scale", "-0.1"], ["--aug_translate", "0.51"],
                ["--aug_translate", "-0.2"]):
        with pytest.raises(AssertionError, match=bad[0][2:]):
            finalize(parser.parse_args(bad))                                 # the range checks come before anything that needs a device


def test_library_exports_the_affine_entry_points_and_rejects_bad_arguments():
    """Host-side validation only: nothing below reaches a launch."""
    import ctypes as C
    from structuredetector_amd import _lib as L
    lib = L.lib()
    names = {"sd_preprocess_affine_workspace_bytes", "sd_preprocess_images_affine", "sd_preprocess_images_list_affine"}
    assert names <= set(L.declared_symbols()) and all(hasattr(lib, n) for n in names)
    B, Hin, Win, Hout, Wout = 2, 8, 8, 4, 4
    need = lib.sd_preprocess_affine_workspace_bytes(B, Hin, Win, Hout, Wout)
    assert need == lib.sd_preprocess_jitter_workspace_bytes(B, Hin, Win, Hout, Wout) + 256
    m3, s3, fill = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25), (C.c_ubyte * 3)(*FILL)
    P = 4096
    for fn, name in ((lib.sd_preprocess_images_affine, b"sd_preprocess_images_affine"),
                     (lib.sd_preprocess_images_list_affine, b"sd_preprocess_images_list_affine")):
        def call(order=P, factors=P, affine=P, ws=need):
            return fn(P, B, Hin, Win, Hout, Wout, P, P, 3, P, P, 3, 0, order, factors, affine, fill, m3, s3, P, P, ws, 0)
        for what, kw, code in (("null affine", dict(affine=None), -1), ("order without factors", dict(factors=None), -1),
                               ("factors without order", dict(order=None), -1), ("short workspace", dict(ws=need - 1), -2),
                               ("short workspace, no jitter", dict(order=None, factors=None, ws=need - 1), -2)):
            lib.sd_set_option(b"no_such_option", 1)
            assert call(**kw) == code, f"{name.decode()}: {what}"
            assert name in lib.sd_last_error(), f"{name.decode()}: {what}: {lib.sd_last_error()}"
