"""Mosaic augmentation (`--aug_mosaic P`), the parts that need no GPU: the table builder, the random draws, the annotation rule, the
composite's definition (tests/affine_ref.py's restatement against Pillow's four transforms + quadrant select), the image / annotation
consistency, the flag and the C entry points' argument checks."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.affine_ref import FILL, blob_image
from tests.mosaic_ref import numpy_mosaic, pil_mosaic, quadrants

IDENT = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def _annotation(objects, path="a.png"):
    from structuredetector_amd.utils import Box, ImageAnnotation, Keypoint, Object
    return ImageAnnotation(path, [Object(name, Keypoint("stem", *anchor), [Keypoint("leaf", *p) for p in parts], Box(*box) if box else None)
                                  for name, anchor, parts, box in objects], img_size=(64, 32))


def _flat(ann):
    return [(o.name, (o.x, o.y), [(p.x, p.y) for p in o.parts]) for o in ann.objects]


def test_table_builder_rows_matrices_and_rectangles():
    from structuredetector_amd.data import mosaic_tiles
    for W, H in ((64, 32), (128, 96), (512, 512)):
        geom, inv, fwd, rects = mosaic_tiles((W, H), 5, None)
        assert geom[:3] == [W, H, 5] and len(geom) == 6 and all(0 <= s for s in geom[2:])
        assert inv[0] == IDENT and fwd[0] == IDENT and rects[0] == (0, 0, W, H)
        assert all(x0 >= x1 or y0 >= y1 for x0, y0, x1, y1 in rects[1:])        # the other tiles own nothing
        for cx, cy in ((W // 4, H // 4), (W // 2, H // 2), (W // 2 + 3, H // 2 - 5), (3 * W // 4, 3 * H // 4), (W // 4, 3 * H // 4)):
            geom, inv, fwd, rects = mosaic_tiles((W, H), 2, (cx, cy, (7, 2, 9)))
            assert geom == [cx, cy, 2, 7, 2, 9]
            own = np.full((H, W), -1)
            q = quadrants(H, W, cx, cy)
            for k in range(4):
                ox = cx - W // 2 if k in (0, 2) else cx
                oy = cy - H // 2 if k < 2 else cy
                assert inv[k] == [2, 0, -2 * ox, 0, 2, -2 * oy] and all(isinstance(v, float) for v in inv[k])
                assert fwd[k] == [0.5, 0, ox, 0, 0.5, oy]
                I3, F3 = np.array([inv[k][:3], inv[k][3:], [0, 0, 1]]), np.array([fwd[k][:3], fwd[k][3:], [0, 0, 1]])
                assert np.array_equal(F3 @ I3, np.eye(3))                       # exact: powers of two and integers
                x0, y0, x1, y1 = rects[k]
                assert 0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H
                assert (own[y0:y1, x0:x1] == -1).all()                          # disjoint
                own[y0:y1, x0:x1] = k
                assert (q[y0:y1, x0:x1] == k).all()                             # inside its quadrant
                # the rectangle is exactly where the tile's matrix lands inside the source, within its quadrant
                xin = 2 * (np.arange(W) + 0.5) - 2 * ox
                yin = 2 * (np.arange(H) + 0.5) - 2 * oy
                shown = ((xin >= 0) & (xin < W))[None, :] & ((yin >= 0) & (yin < H))[:, None] & (q == k)
                assert np.array_equal(shown, own == k)
            if (cx, cy) == (W // 2, H // 2):
                assert (own >= 0).all()                                         # a central cut: the four half images tile the canvas
            else:
                assert (own >= 0).sum() == min(cx, W // 2) * min(cy, H // 2) + min(W - cx, W // 2) * min(cy, H // 2) \
                    + min(cx, W // 2) * min(H - cy, H // 2) + min(W - cx, W // 2) * min(H - cy, H // 2)


def test_draws_are_reproducible_in_range_and_stay_in_the_group():
    from structuredetector_amd.data import TrainAugmentation
    args = Namespace(width=128, height=96, no_augmentation=False, device=None, aug_mosaic=0.5)
    aug = TrainAugmentation(args)
    n = 2048
    groups = [[i for i in range(n) if i % 3 == 0], [i for i in range(n) if i % 3 == 1], [i for i in range(n) if i % 3 == 2][:5],
              [i for i in range(n) if i % 3 == 2][5:]]
    member = {i: set(idx) for idx in groups for i in idx}
    torch.manual_seed(11)
    before = torch.get_rng_state()
    a = aug.mosaic_draws_for(n, groups)
    after = torch.get_rng_state()
    torch.manual_seed(11)
    assert aug.mosaic_draws_for(n, groups) == a
    torch.set_rng_state(before)
    u = torch.rand(n, 6, dtype=torch.float64)                                   # ONE draw of this shape, nothing else
    assert torch.equal(torch.get_rng_state(), after)
    assert len(a) == n
    picked = [i for i in range(n) if a[i] is not None]
    assert picked == [i for i in range(n) if u[i, 0] < 0.5] and 0.4 * n < len(picked) < 0.6 * n
    cxs, cys = set(), set()
    for i in picked:
        cx, cy, partners = a[i]
        assert isinstance(cx, int) and isinstance(cy, int) and 32 <= cx <= 96 and 24 <= cy <= 72
        assert len(partners) == 3 and all(p in member[i] for p in partners)
        assert partners == tuple(sorted(member[i])[int(v * len(member[i]))] for v in u[i, 3:].tolist())
        cxs.add(cx); cys.add(cy)
    assert cxs == set(range(32, 97)) and cys == set(range(24, 73))              # both ends of the range are reached
    assert any(i in a[i][2] for i in picked) and any(len(set(a[i][2])) < 3 for i in picked)     # itself, and repeats, are allowed
    aug.size = (160, 64)                                                        # the centre follows the multi-scale size
    b = [d for d in aug.mosaic_draws_for(n, groups) if d is not None]
    assert min(d[0] for d in b) == 40 and max(d[0] for d in b) == 120 and min(d[1] for d in b) == 16 and max(d[1] for d in b) == 48
    every = TrainAugmentation(Namespace(**{**vars(args), "aug_mosaic": 1.0})).mosaic_draws_for(64, [list(range(64))])
    assert all(d is not None for d in every)


def test_draws_off_consume_nothing():
    from structuredetector_amd.data import TrainAugmentation, ValidationAugmentation
    groups = [list(range(64))]
    torch.manual_seed(7)
    before = torch.get_rng_state()
    assert TrainAugmentation(Namespace(width=128, height=96, no_augmentation=False, device=None, aug_mosaic=0.0)).mosaic_draws_for(64, groups) is None
    assert TrainAugmentation(Namespace(width=128, height=96, no_augmentation=False, device=None)).mosaic_draws_for(64, groups) is None
    on = Namespace(width=128, height=96, no_augmentation=False, device=None, aug_mosaic=0.5)
    assert ValidationAugmentation(on).mosaic_draws_for(64, groups) is None
    assert TrainAugmentation(Namespace(**{**vars(on), "no_augmentation": True})).mosaic_draws_for(64, groups) is None
    assert torch.equal(torch.get_rng_state(), before)
    assert TrainAugmentation(on).mosaic_draws_for(64, groups) is not None and not torch.equal(torch.get_rng_state(), before)


def test_mosaic_annotation_on_a_hand_made_scene():
    """64 x 32 canvas cut at (40, 12).  Tile origins: q0 (8, -4), q1 (40, -4), q2 (8, 12), q3 (40, 12); a point p lands at p / 2 + o - 0.25.
    Rectangles (pixel ownership, x0 <= x' + 0.5 < x1): q0 (8, 0, 40, 12), q1 (40, 0, 64, 12), q2 (8, 12, 40, 28), q3 (40, 12, 64, 28)."""
    from structuredetector_amd.data import mosaic_tiles
    from structuredetector_amd.utils import mosaic_annotation
    geom, _, fwd, rects = mosaic_tiles((64, 32), 0, (40, 12, (1, 2, 1)))
    assert rects == [(8, 0, 40, 12), (40, 0, 64, 12), (8, 12, 40, 28), (40, 12, 64, 28)]
    a0 = _annotation([("a-in", (20.0, 20.0), [(62.0, 30.0), (63.0, 31.0), (63.0, 31.5), (10.0, 7.0)], (10.0, 10.0, 30.0, 28.0)),    # y 31.5 -> 11.5, + 0.5 = 12: out; y 7 -> -0.75: out
                      ("a-out", (30.0, 6.0), [(20.0, 20.0)], None)], "zero.png")                                       # anchor y -> -1.25: out
    a1 = _annotation([("b-in", (0.0, 8.0), [(46.0, 10.0), (48.0, 10.0)], None),                                       # q1: x 48 -> 63.75: out
                      ("b-both", (10.0, 20.0), [(2.0, 30.0)], None)], "one.png")                                      # kept by q1, part y 30 -> 10.75: in
    a2 = _annotation([("c-in", (63.0, 0.0), [(0.0, 0.0), (63.5, 31.0)], None),                                        # q2: part (0, 0) -> (7.75, 11.75): in
                      ("c-out", (5.0, 31.9), [], None)], "two.png")                                                   # y -> 27.7, + 0.5 = 28.2 >= 28: out
    sources = [a0, a1, a2, a1]
    before = [_flat(s) for s in (a1, a2)]
    target = a0                                                                 # image 0 is its own tile 0
    snapshot = [Namespace(objects=list(s.objects)) for s in sources]
    mosaic_annotation(target, snapshot, fwd, rects)
    assert [_flat(s) for s in (a1, a2)] == before                                # the partners are untouched
    assert target.image_path.name == "zero.png" and target.img_size == (64, 32)
    got = _flat(target)
    want = [("a-in", (17.75, 5.75), [(38.75, 10.75), (39.25, 11.25)]),           # tile 0: p / 2 + (8, -4) - 0.25
            ("b-in", (39.75, -0.25), [(62.75, 0.75)]),                          # tile 1: p / 2 + (40, -4) - 0.25
            ("b-both", (44.75, 5.75), [(40.75, 10.75)]),
            ("c-in", (39.25, 11.75), [(7.75, 11.75)]),                          # tile 2: p / 2 + (8, 12) - 0.25; part x 63.5 -> 39.5 + 0.5 = 40: out
            ("b-in", (39.75, 15.75), [(62.75, 16.75)]),                         # tile 3: p / 2 + (40, 12) - 0.25
            ("b-both", (44.75, 21.75), [(40.75, 26.75)])]
    assert got == want, got
    box = target.objects[0].box
    assert (box.x_min, box.y_min, box.x_max, box.y_max) == (12.75, 0.75, 22.75, 9.75)          # the hull of the moved corners
    assert target.objects[1].anchor is not a1.objects[0].anchor and target.objects[1] is not target.objects[4]     # clones, one per tile
    # the same image as three tiles and edited afterwards: the sources must not follow
    target.objects[1].x = -100.0
    assert a1.objects[0].x == 0.0 and target.objects[4].x == 39.75
    # an empty tile (centre at the origin: tile 3 only)
    geom, _, fwd, rects = mosaic_tiles((64, 32), 0, (0, 0, (1, 1, 1)))
    t = _annotation([("gone", (10.0, 10.0), [], None)])
    mosaic_annotation(t, [t, a1, a1, a1], fwd, rects)
    assert [o.name for o in t.objects] == ["b-in", "b-both"] and (t.objects[0].x, t.objects[0].y) == (-0.25, 3.75)


@pytest.mark.parametrize("size", [(64, 32), (70, 33)])
def test_numpy_composite_equals_the_pillow_composite(size):
    from structuredetector_amd.data import mosaic_tiles
    from structuredetector_amd.data.augment import _FILL, affine_inverse_matrix
    assert _FILL == FILL
    W, H = size
    rng = np.random.default_rng(W)
    imgs = rng.integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    centres = [(W // 4, H // 4), (W // 2 + 3, H // 2 + 1), (3 * W // 4, 3 * H // 4), (W // 2 - 3, H // 4), (0, H // 2), (W, H // 2), (0, 0), (W, H)]
    assert any(cx % 4 for cx, _ in centres)
    filled = 0
    for cx, cy in centres:
        geom, inv, _, rects = mosaic_tiles(size, 0, (cx, cy, (1, 2, 3)))
        want = pil_mosaic(imgs, geom, inv)
        got = numpy_mosaic(imgs, geom, inv)
        assert np.array_equal(got, want), f"{size} centre {(cx, cy)}: {(got != want).any(-1).sum()} pixels differ"
        own = np.zeros((H, W), bool)
        for x0, y0, x1, y1 in rects:
            own[y0:y1, x0:x1] = True
        assert (want[~own] == np.asarray(FILL, np.uint8)).all()                 # what no tile owns is fill
        filled += (~own).sum()
        # a policy tap is a 2 x 2 block mean, truncated
        x0, y0, x1, y1 = rects[3]
        if x1 > x0 and y1 > y0:
            blk = imgs[3][0:2, 0:2].astype(np.float64)
            assert np.array_equal(want[y0, x0], np.floor(blk.sum((0, 1)) / 4).astype(np.uint8))         # halves and quarters: exact in double
    assert filled > 0
    geom, inv, _, _ = mosaic_tiles(size, 2, None)                               # not selected: a copy of image s0
    assert np.array_equal(pil_mosaic(imgs, geom, inv), imgs[2]) and np.array_equal(numpy_mosaic(imgs, geom, inv), imgs[2])
    general = [affine_inverse_matrix(size, 10.0, 0.37, (3.0, -2.0)), [1.7, 0.0, -5.0, 0.0, 0.6, 2.5], inv[0], [2.0, 0.0, -7.0, 0.0, 2.0, -3.0]]
    g = [W // 4 + 1, 3 * H // 4, 3, 1, 0, 1]
    assert np.array_equal(numpy_mosaic(imgs, g, general), pil_mosaic(imgs, g, general))


def test_image_and_annotation_conventions_agree():
    """A 3 x 3 blob on one keypoint of each of four sources: in the composite, the blob lies within 1 pixel of where mosaic_annotation puts
    the keypoint."""
    from structuredetector_amd.data import mosaic_tiles
    from structuredetector_amd.utils import mosaic_annotation
    W, H = 64, 32
    points = [(40, 20), (11, 9), (50, 7), (20, 16)]                             # one per source, each inside the part of it its tile shows
    imgs = [blob_image(H, W, [p]) for p in points]
    geom, inv, fwd, rects = mosaic_tiles((W, H), 0, (35, 13, (1, 2, 3)))
    out = pil_mosaic(imgs, geom, inv)[..., 0].astype(np.float64) - FILL[0]
    anns = [_annotation([(f"o{k}", (float(x), float(y)), [], None)]) for k, (x, y) in enumerate(points)]
    target = mosaic_annotation(anns[0], [Namespace(objects=list(a.objects)) for a in anns], fwd, rects)
    assert [o.name for o in target.objects] == ["o0", "o1", "o2", "o3"]
    for k, o in enumerate(target.objects):
        x0, y0, x1, y1 = rects[k]
        wgt = np.zeros_like(out)
        wgt[y0:y1, x0:x1] = np.clip(out[y0:y1, x0:x1], 0, None)                 # what is brighter than the fill, inside the tile
        assert wgt.max() == 255 - FILL[0]                                       # a 3-wide blob always holds one whole 2 x 2 block
        bx = (wgt * np.arange(W)[None, :]).sum() / wgt.sum()
        by = (wgt * np.arange(H)[:, None]).sum() / wgt.sum()
        assert np.hypot(bx - o.x, by - o.y) <= 1.0, (k, (bx, by), (o.x, o.y))


def test_flag_parses_defaults_off_and_validates():
    from structuredetector_amd.utils.args import Arguments, finalize
    parser = Arguments().parser
    assert parser.parse_args([]).aug_mosaic == 0.0
    assert parser.parse_args(["--aug_mosaic", "0.5"]).aug_mosaic == 0.5
    text = " ".join(parser.format_help().split())
    assert "--aug_mosaic P" in text and "--max_objects" in text.split("--aug_mosaic P")[1] and "--max_parts" in text.split("--aug_mosaic P")[1]
    for bad in ("-0.1", "1.01", "2"):
        with pytest.raises(AssertionError, match="aug_mosaic"):
            finalize(parser.parse_args(["--aug_mosaic", bad]))                  # the range check comes before anything that needs a device


def test_library_exports_the_mosaic_entry_points_and_rejects_bad_arguments():
    """Host-side validation only: nothing below reaches a launch."""
    import ctypes as C
    from structuredetector_amd import _lib as L
    lib = L.lib()
    names = {"sd_preprocess_mosaic_workspace_bytes", "sd_preprocess_images_mosaic", "sd_preprocess_images_list_mosaic"}
    assert names <= set(L.declared_symbols()) and all(hasattr(lib, n) for n in names)
    B, Hin, Win, Hout, Wout = 2, 8, 8, 4, 4
    need = lib.sd_preprocess_mosaic_workspace_bytes(B, Hin, Win, Hout, Wout)
    assert need == lib.sd_preprocess_affine_workspace_bytes(B, Hin, Win, Hout, Wout)      # two 8-bit images serve all four chains
    m3, s3, fill = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25), (C.c_ubyte * 3)(*FILL)
    P = 4096
    for fn, name in ((lib.sd_preprocess_images_mosaic, b"sd_preprocess_images_mosaic"),
                     (lib.sd_preprocess_images_list_mosaic, b"sd_preprocess_images_list_mosaic")):
        def call(order=P, factors=P, affine=P, geom=P, mats=P, ws=need):
            return fn(P, B, Hin, Win, Hout, Wout, P, P, 3, P, P, 3, 0, order, factors, affine, geom, mats, fill, m3, s3, P, P, ws, 0)
        for what, kw, code in (("null geometry", dict(geom=None), -1), ("null matrices", dict(mats=None), -1),
                               ("order without factors", dict(factors=None), -1), ("factors without order", dict(order=None), -1),
                               ("short workspace", dict(ws=need - 1), -2),
                               ("short workspace, no warp, no jitter", dict(order=None, factors=None, affine=None, ws=need - 1), -2)):
            lib.sd_set_option(b"no_such_option", 1)
            assert call(**kw) == code, f"{name.decode()}: {what}"
            assert name in lib.sd_last_error(), f"{name.decode()}: {what}: {lib.sd_last_error()}"
