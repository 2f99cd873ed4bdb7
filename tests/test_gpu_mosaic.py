"""Mosaic augmentation on the GPU (sd_preprocess_images_mosaic / _list_mosaic: k_mosaic_u8, k_mosaic_norm) against Pillow itself:
F.resize (PIL) -> four Image.transform(AFFINE, BILINEAR, fillcolor) + quadrant select -> [RandomAffine] -> [ColorJitter] -> flips ->
to_tensor -> Normalize, bit for bit; the list form against the packed form; the fused kernel against the staged one; the table clamps;
TrainAugmentation end to end with the annotations; a few training steps."""
import ctypes as C
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.affine_ref import FILL, PARAMS, pil_affine
from tests.mosaic_ref import FLIPS, batch_tables, clamped, pil_mosaic
from tests.test_gpu_pipeline import MEAN, STD, pil_color_jitter

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 6
SIZES = [(64, 32), (96, 64), (70, 33)]          # (70, 33): a width that is no multiple of 4 (the byte-store branch) and a partial block
SOURCES = [(33, 47), (160, 96)]


@functools.lru_cache(maxsize=None)
def _case(src, size):
    """Images, tables, the Pillow-resized images and the Pillow composites of one (source size, output size): computed once, read only."""
    from PIL import Image
    rng = np.random.default_rng(src[0] * 131 + size[0])
    imgs = rng.integers(0, 256, (B, src[0], src[1], 3), dtype=np.uint8)
    geom, mats = batch_tables(size)
    resized = [np.asarray(Image.fromarray(im).resize(size, Image.BILINEAR)).copy() for im in imgs]
    composites = [pil_mosaic(resized, geom[b], mats[b]) for b in range(B)]
    for a in (imgs, *resized, *composites):
        a.setflags(write=False)
    return imgs, geom, mats, resized, composites


def _finish(u8, flip, jit=None):
    """[ColorJitter] -> flips -> to_tensor -> Normalize of an (H, W, 3) uint8 image, on PIL images."""
    from PIL import Image
    im = Image.fromarray(u8)
    if jit is not None:
        im = pil_color_jitter(im, *jit)
    if flip & 1:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if flip & 2:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    t = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).to(torch.float32).div(255)
    return t.sub(MEAN).div(STD)


def _warps(size):
    from structuredetector_amd.data.augment import affine_inverse_matrix
    return [affine_inverse_matrix(size, a, s, (tx, ty)) for a, s, tx, ty in PARAMS[1:1 + B]]


def _random_jitter(rng, n):
    from structuredetector_amd.data.augment import jitter_words
    jit = [jitter_words(list(rng.permutation(4)), *rng.uniform(0.75, 1.25, 2), rng.uniform(0.85, 1.15), rng.uniform(-0.05, 0.05)) for _ in range(n)]
    return [w for w, _ in jit], [f for _, f in jit]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("src", SOURCES)
def test_mosaic_matches_pillow_bitwise(src, size):
    from structuredetector_amd.data import preprocess_images
    imgs, geom, mats, _, composites = _case(src, size)
    got = preprocess_images(torch.tensor(imgs, device=DEV), size, FLIPS, mosaic=(geom, mats)).cpu()
    assert got.shape == (B, 3, size[1], size[0])
    for b in range(B):
        want = _finish(composites[b], FLIPS[b])
        assert torch.equal(got[b], want), f"image {b} {geom[b]} flips {FLIPS[b]}: {(got[b] != want).sum().item()} values differ"
    unflipped = preprocess_images(torch.tensor(imgs, device=DEV), size, mosaic=(geom, mats)).cpu()             # flips = None
    assert torch.equal(unflipped[3], _finish(composites[3], 0))
    fill = ((torch.tensor(FILL, dtype=torch.float32) / 255)[:, None, None] - MEAN) / STD
    assert (got[1] == fill).all(0).float().mean() > 0.5                                                          # tile 3 only: mostly fill


@pytest.mark.parametrize("order", [[1, 0, 2, 3], [0, 2, 3, 1]], ids=["contrast_first", "contrast_last"])
@pytest.mark.parametrize("src,size", [((33, 47), (96, 64)), ((160, 96), (64, 32)), ((160, 96), (70, 33))])
def test_mosaic_then_affine_then_jitter_matches_pillow_bitwise(src, size, order):
    """The contrast op blends with the grey mean of the COMPOSED and WARPED image.  Also mosaic -> jitter and mosaic -> warp."""
    from structuredetector_amd.data import preprocess_images
    from structuredetector_amd.data.augment import jitter_words
    imgs, geom, mats, _, composites = _case(src, size)
    warps = _warps(size)
    rng = np.random.default_rng(5)
    jits = [(order, float(rng.uniform(0.75, 1.25)), float(rng.uniform(0.75, 1.25)), float(rng.uniform(0.85, 1.15)), float(rng.uniform(-0.05, 0.05)))
            for _ in range(B)]
    words, factors = zip(*(jitter_words(*j) for j in jits))
    jitter = (list(words), list(factors))
    x = torch.tensor(imgs, device=DEV)
    full = preprocess_images(x, size, FLIPS, jitter=jitter, affine=warps, mosaic=(geom, mats)).cpu()
    no_warp = preprocess_images(x, size, FLIPS, jitter=jitter, mosaic=(geom, mats)).cpu()
    no_jitter = preprocess_images(x, size, FLIPS, affine=warps, mosaic=(geom, mats)).cpu()
    for b in range(B):
        warped = pil_affine(composites[b], warps[b])
        for name, got, want in (("mosaic, warp, jitter", full, _finish(warped, FLIPS[b], jits[b])),
                                ("mosaic, jitter", no_warp, _finish(composites[b], FLIPS[b], jits[b])),
                                ("mosaic, warp", no_jitter, _finish(warped, FLIPS[b]))):
            assert torch.equal(got[b], want), f"{name}: image {b} {geom[b]} {PARAMS[1 + b]}: {(got[b] != want).sum().item()} values differ"


def test_list_form_equals_the_packed_form():
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    from tests.test_gpu_image_cache import _arena_with
    rng = np.random.default_rng(21)
    hin, win = 37, 53
    imgs = [rng.integers(0, 256, (hin, win, 3), dtype=np.uint8) for _ in range(3)]
    arena, addrs = _arena_with(imgs, rng)
    assert all(a % 2 == 1 for a in addrs)                                       # unaligned
    order = [2, 0, 2, 1, 0, 1]                                                  # duplicate pointers
    table = torch.tensor([addrs[t] for t in order], dtype=torch.int64, device=DEV)
    packed = torch.from_numpy(np.stack([imgs[t] for t in order])).to(DEV)
    jitter = _random_jitter(rng, B)
    for size in ((96, 64), (70, 33)):
        mosaic, warps = batch_tables(size), _warps(size)
        for jit in (None, jitter):
            for warp in (None, warps):
                want = preprocess_images(packed, size, FLIPS, jitter=jit, affine=warp, mosaic=mosaic)
                got = preprocess_image_list(table, hin, win, size, FLIPS, jitter=jit, affine=warp, mosaic=mosaic)
                assert got.shape == (B, 3, size[1], size[0]) and torch.equal(got, want), (size, jit is not None, warp is not None)
    torch.cuda.synchronize()
    del arena


@pytest.mark.parametrize("size", SIZES)
def test_fused_kernel_equals_the_u8_kernel_and_an_identity_warp(size):
    """k_mosaic_norm against k_mosaic_u8 followed by k_affine_norm with identity matrices (exact bytes: test_identity_matrices_change_nothing)."""
    from structuredetector_amd.data import preprocess_images
    imgs, geom, mats, _, _ = _case((160, 96), size)
    x = torch.tensor(imgs, device=DEV)
    ident = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * B
    for flips in (None, FLIPS):
        assert torch.equal(preprocess_images(x, size, flips, mosaic=(geom, mats)), preprocess_images(x, size, flips, affine=ident, mosaic=(geom, mats)))


def test_an_all_non_selected_table_is_the_parent_path():
    from structuredetector_amd.data import mosaic_tiles, preprocess_images
    rng = np.random.default_rng(9)
    imgs = torch.from_numpy(rng.integers(0, 256, (B, 75, 50, 3), dtype=np.uint8)).to(DEV)
    jitter = _random_jitter(rng, B)
    for size in ((96, 64), (70, 33)):
        rows = [mosaic_tiles(size, b, None) for b in range(B)]
        mosaic = ([r[0] for r in rows], [r[1] for r in rows])
        warps = _warps(size)
        for flips in (None, FLIPS):
            assert torch.equal(preprocess_images(imgs, size, flips, jitter=jitter, mosaic=mosaic), preprocess_images(imgs, size, flips, jitter=jitter))
            assert torch.equal(preprocess_images(imgs, size, flips, mosaic=mosaic), preprocess_images(imgs, size, flips))
            assert torch.equal(preprocess_images(imgs, size, flips, jitter=jitter, affine=warps, mosaic=mosaic),
                               preprocess_images(imgs, size, flips, jitter=jitter, affine=warps))
            assert torch.equal(preprocess_images(imgs, size, flips, affine=warps, mosaic=mosaic), preprocess_images(imgs, size, flips, affine=warps))


@pytest.mark.parametrize("size", [(96, 64), (70, 33)])
def test_out_of_range_table_entries_are_clamped(size):
    """The memory-safety contract: the device tables cannot be checked on the host, so the kernels clamp sources to [0, B) and the centre
    to [0, W] x [0, H]; the output is that of the clamped table."""
    from structuredetector_amd.data import preprocess_images
    W, H = size
    imgs, geom, mats, _, _ = _case((160, 96), size)
    x = torch.tensor(imgs, device=DEV)
    wild = [list(g) for g in geom]
    wild[0][3], wild[0][4] = -1, B                                              # sources below and above the batch
    wild[3][0], wild[3][5] = W + 5, B + 1000
    wild[4][0], wild[4][1] = -1, H + 5
    wild[5][1], wild[5][2] = -7, -2**31
    tame = [clamped(g, B, W, H) for g in wild]
    assert tame != wild and all(0 <= g[0] <= W and 0 <= g[1] <= H and all(0 <= s < B for s in g[2:]) for g in tame)
    jitter = _random_jitter(np.random.default_rng(2), B)
    for jit in (None, jitter):
        got = preprocess_images(x, size, FLIPS, jitter=jit, mosaic=(wild, mats))
        torch.cuda.synchronize()                                                # the call and the launches succeeded
        assert torch.equal(got, preprocess_images(x, size, FLIPS, jitter=jit, mosaic=(tame, mats))), jit is not None


def test_c_abi_rejects_bad_arguments_before_any_launch():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    Bn, Hin, Win, Hout, Wout = 2, 8, 8, 4, 4
    need = lib.sd_preprocess_mosaic_workspace_bytes(Bn, Hin, Win, Hout, Wout)
    m3, s3, fill = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25), (C.c_ubyte * 3)(*FILL)
    P = 4096                                                                   # never dereferenced: no call below reaches a launch
    for fn, name in ((lib.sd_preprocess_images_mosaic, b"sd_preprocess_images_mosaic"),
                     (lib.sd_preprocess_images_list_mosaic, b"sd_preprocess_images_list_mosaic")):
        def call(order=P, factors=P, affine=P, geom=P, mats=P, ws=need):
            return fn(P, Bn, Hin, Win, Hout, Wout, P, P, 3, P, P, 3, 0, order, factors, affine, geom, mats, fill, m3, s3, P, P, ws, 0)
        for what, kw, code in (("null geometry", dict(geom=None), -1), ("null matrices", dict(mats=None), -1),
                               ("order without factors", dict(factors=None), -1), ("factors without order", dict(order=None), -1),
                               ("workspace one byte short", dict(ws=need - 1), -2),
                               ("workspace one byte short, no warp", dict(affine=None, ws=need - 1), -2)):
            lib.sd_set_option(b"no_such_option", 1)                            # leaves another message behind
            assert call(**kw) == code, f"{name.decode()}: {what}"
            assert lib.sd_last_error() and name in lib.sd_last_error(), f"{name.decode()}: {what}: {lib.sd_last_error()}"


# ---- TrainAugmentation end to end -----------------------------------------------------------------------------------------------
SRC_H, SRC_W, OUT_W, OUT_H = 192, 256, 128, 96


def layout(i):
    """Scene i: five objects, one per column of a 5 x 3 grid (50 x 64 source pixels apart = 12.5 x 16 in a tile), shifted by (4 i, 2 i); the
    anchor of object k sits in row (k + i) % 3, its two parts in the other rows.  Even coordinates: a 12 x 12 source blob becomes 6 x 6 in
    the resized image and 3 x 3 in a tile, centred on the keypoint."""
    objects = []
    for k in range(5):
        pts = [(28 + 50 * k + 4 * i, 30 + 64 * r + 2 * i) for r in range(3)]
        anchor = pts.pop((k + i) % 3)
        objects.append((anchor, pts))
    return objects


def scene(i):
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    img = np.zeros((SRC_H, SRC_W, 3), np.uint8)
    objects = []
    for k, (anchor, parts) in enumerate(layout(i)):
        for x, y in (anchor, *parts):
            img[y - 5:y + 7, x - 5:x + 7] = 255                                  # pixels x - 5 .. x + 6: centred on index x + 0.5, resized index x / 2
        objects.append(Object(f"i{i}o{k}", Keypoint("stem", float(anchor[0]), float(anchor[1])),
                              [Keypoint(f"p{j}", float(x), float(y)) for j, (x, y) in enumerate(parts)]))
    return img, ImageAnnotation(f"s{i}.png", objects)


def expected_annotations(i, mosaics, warps, flips):
    """The host rule written out for image i: resize, tile (kept iff the tile owns the point), warp about the centre (kept iff inside), flips,
    clip.  Returns ([(name, [(x, y) of the anchor and the kept parts])] in tile order, number of dropped keypoints)."""
    cx, cy, partners = mosaics[i]
    dropped = 0

    def tile_rule(q, x, y):
        ox = cx - OUT_W // 2 if q in (0, 2) else cx
        oy = cy - OUT_H // 2 if q < 2 else cy
        x0, x1 = (max(ox, 0), cx) if q in (0, 2) else (cx, min(ox + OUT_W // 2, OUT_W))
        y0, y1 = (max(oy, 0), cy) if q < 2 else (cy, min(oy + OUT_H // 2, OUT_H))
        X, Y = (x * OUT_W / SRC_W + 0.5) / 2 + ox, (y * OUT_H / SRC_H + 0.5) / 2 + oy          # centre coordinates on the canvas
        if not (x0 <= X < x1 and y0 <= Y < y1):
            return None
        if warps is not None:
            angle, scale, tx, ty = warps[i]
            c, s = np.cos(np.radians(angle)) * scale, np.sin(np.radians(angle)) * scale
            u, v = X - OUT_W / 2, Y - OUT_H / 2
            X, Y = c * u - s * v + OUT_W / 2 + tx, s * u + c * v + OUT_H / 2 + ty
            if not (0 <= X < OUT_W and 0 <= Y < OUT_H):
                return None
        X, Y = X - 0.5, Y - 0.5
        if flips[i] & 1:
            X = OUT_W - X - 1
        if flips[i] & 2:
            Y = OUT_H - Y - 1
        return min(max(X, 0), OUT_W - 1), min(max(Y, 0), OUT_H - 1)                           # clip_annotation

    expect = []
    for q, s in enumerate((i, *partners)):
        for k, (anchor, parts) in enumerate(layout(s)):
            a = tile_rule(q, *anchor)
            if a is None:
                dropped += 1 + len(parts)
                continue
            kept = [p for p in (tile_rule(q, *p) for p in parts) if p is not None]
            dropped += len(parts) - len(kept)
            expect.append((f"i{s}o{k}", [a] + kept))
    return expect, dropped


def _peak_near(plane, x, y, radius=4):
    """Centre of the brightest plateau in the window around (x, y)."""
    H, W = plane.shape
    x0, x1, y0, y1 = max(int(round(x)) - radius, 0), min(int(round(x)) + radius + 1, W), max(int(round(y)) - radius, 0), min(int(round(y)) + radius + 1, H)
    win = plane[y0:y1, x0:x1]
    ys, xs = np.nonzero(win >= win.max() - 1e-6)
    return x0 + xs.mean(), y0 + ys.mean(), win.max()


def check_end_to_end(out, anns, mosaics, warps, flips):
    """Annotations equal the rule; every kept keypoint has an image peak within 1.5 pixels.  Returns (kept, dropped)."""
    kept = dropped = 0
    for i in range(4):
        expect, d = expected_annotations(i, mosaics, warps, flips)
        dropped += d
        got = [(o.name, [(o.x, o.y)] + [(p.x, p.y) for p in o.parts]) for o in anns[i].objects]
        assert [n for n, _ in got] == [n for n, _ in expect] and all(len(g[1]) == len(e[1]) for g, e in zip(got, expect)), (i, got, expect)
        assert anns[i].image_path.name == f"s{i}.png"
        plane = out[i].sum(0)
        for (n, gp), (_, ep) in zip(got, expect):
            for (gx, gy), (ex, ey) in zip(gp, ep):
                assert abs(gx - ex) <= 1e-9 and abs(gy - ey) <= 1e-9, (i, n, (gx, gy), (ex, ey))
                px, py, peak = _peak_near(plane, gx, gy)
                assert peak > plane.min() + 3.0 and np.hypot(px - gx, py - gy) <= 1.5, (i, n, (gx, gy), (px, py), peak)
                kept += 1
    return kept, dropped


@pytest.mark.parametrize("warp", [False, True], ids=["mosaic", "mosaic_and_warp"])
def test_train_augmentation_moves_images_and_annotations_together(warp):
    from structuredetector_amd.data import TrainAugmentation
    extra = dict(aug_rotate=20.0, aug_scale=0.15, aug_translate=0.05) if warp else {}
    args = Namespace(width=OUT_W, height=OUT_H, no_augmentation=False, device=torch.device(DEV), aug_mosaic=1.0, **extra)
    aug = TrainAugmentation(args)
    torch.manual_seed(9)
    flips, _ = aug.draws_for(4)
    warps = aug.affine_draws_for(4)                                            # the draws the call below makes, in its order
    mosaics = aug.mosaic_draws_for(4, [[0, 1, 2, 3]])
    assert (warps is not None) == warp and all(m is not None for m in mosaics)
    torch.manual_seed(9)
    out, anns = aug([scene(i)[0] for i in range(4)], [scene(i)[1] for i in range(4)])
    assert out.shape == (4, 3, OUT_H, OUT_W)
    kept, dropped = check_end_to_end(out.cpu().numpy(), anns, mosaics, warps, flips)
    assert dropped >= 2 and kept >= 20, (dropped, kept)


def test_train_augmentation_with_the_flag_off_is_the_parent_path():
    from structuredetector_amd.data import TrainAugmentation, preprocess_images
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (60, 80, 3), dtype=np.uint8) for _ in range(4)]
    for extra in (dict(), dict(aug_mosaic=0.0)):
        aug = TrainAugmentation(Namespace(width=128, height=96, no_augmentation=False, device=torch.device(DEV), **extra))
        torch.manual_seed(5)
        flips, jitter = aug.draws_for(4)
        state = torch.get_rng_state()
        want = preprocess_images(torch.from_numpy(np.stack(imgs)).to(DEV), (128, 96), flips, jitter=jitter)
        torch.manual_seed(5)
        got, anns = aug(imgs, [scene(0)[1] for _ in range(4)])
        assert torch.equal(torch.get_rng_state(), state) and torch.equal(got, want)
        assert all(len(a.objects) == 5 and a.nb_parts == 10 for a in anns)       # nothing is composed or dropped


def test_a_few_training_steps_with_mosaic_on():
    """TrainAugmentation(aug_mosaic = 1) -> Encode -> TrainStep at the smoke test's size: finite losses, and no sample over the target
    capacity (a mosaic carries up to four images' objects: max_objects / max_parts are sized for that here)."""
    from structuredetector_amd.data import Encode, TrainAugmentation
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    dev = torch.device("cuda:0")
    labels, parts = {"bean": 0, "maize": 1}, {"p0": 0, "p1": 1}
    args = Namespace(labels=labels, parts=parts, _r_labels={v: k for k, v in labels.items()}, _r_parts={v: k for k, v in parts.items()},
                     anchor_name="stem", down_ratio=4.0, max_objects=20, max_parts=40, conf_threshold=0.5, decoder_dist_thresh=0.1,
                     sigma_gauss=0.1, hm_loss_fn="mse", hm_weight=1.0, offset_weight=0.001, embedding_weight=0.001, fpn_depth=128,
                     learning_rate=1e-3, device=dev, width=128, height=128, no_augmentation=False, aug_mosaic=1.0)
    aug = TrainAugmentation(args)
    net = Network(args, pretrained=False).to(dev).train()
    step = TrainStep(net, args)
    enc = Encode(args)
    torch.manual_seed(3)
    composed = 0
    for _ in range(3):
        x, anns = aug([scene(i)[0] for i in range(4)], [scene(i)[1] for i in range(4)])
        assert all(len(a.objects) <= args.max_objects and a.nb_parts <= args.max_parts for a in anns)
        composed += sum(len({o.name[:2] for o in a.objects}) > 1 for a in anns)
        for a in anns:
            for o in a.objects:
                o.name = "bean" if o.name[1] in "02" else "maize"                # the scenes name objects after their source: give them labels
        loss = step(x, enc.batch((128, 128), anns)).cpu().numpy()
        assert np.isfinite(loss).all(), loss
    assert composed >= 6                                                        # most samples show objects of more than one source
    assert np.isfinite(net.flat_params.cpu().numpy()).all()
