"""Random affine augmentation on the GPU (sd_preprocess_images_affine / _list_affine: k_affine_u8, k_affine_norm) against Pillow itself:
F.resize (PIL) -> Image.transform(AFFINE, BILINEAR, fillcolor) -> [ColorJitter] -> flips -> to_tensor -> Normalize, bit for bit; the list
form against the packed form; TrainAugmentation end to end with the annotations."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.affine_ref import FILL, PARAMS
from tests.test_gpu_pipeline import MEAN, STD, pil_color_jitter

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLIPS = [0, 1, 2, 3, 2, 1, 3]                                                  # one per parameter set: all four codes occur


def reference_chain_affine(img_u8, size, m, hflip, vflip, jit=None):
    """Resize -> RandomAffine -> [ColorJitter] -> flips -> to_tensor -> Normalize on PIL images, torchvision's functional ops written out."""
    from PIL import Image
    im = Image.fromarray(img_u8).resize(size, Image.BILINEAR)
    im = im.transform(size, Image.AFFINE, tuple(m), Image.BILINEAR, fillcolor=FILL)
    if jit is not None:
        im = pil_color_jitter(im, *jit)
    if hflip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if vflip:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    t = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).to(torch.float32).div(255)
    return t.sub(MEAN).div(STD)


def _batch(src, size, seed=0):
    """B = 7 images of one source size, one parameter set each, the matrices computed once on the host at the OUTPUT size."""
    from structuredetector_amd.data.augment import affine_inverse_matrix
    rng = np.random.default_rng(src[0] * 131 + size[0] + seed)
    imgs = rng.integers(0, 256, (len(PARAMS), src[0], src[1], 3), dtype=np.uint8)
    mats = [affine_inverse_matrix(size, a, s, (tx, ty)) for a, s, tx, ty in PARAMS]
    return imgs, mats


# (70, 33): a width that is no multiple of 4 (the byte-store branch), two tiles across with a partial one
@pytest.mark.parametrize("size", [(64, 32), (96, 64), (70, 33)])
@pytest.mark.parametrize("src", [(33, 47), (160, 96)])
def test_affine_matches_pillow_bitwise(src, size):
    from structuredetector_amd.data import preprocess_images
    imgs, mats = _batch(src, size)
    got = preprocess_images(torch.from_numpy(imgs).to(DEV), size, FLIPS, affine=mats).cpu()
    assert got.shape == (7, 3, size[1], size[0])
    for b in range(7):
        want = reference_chain_affine(imgs[b], size, mats[b], bool(FLIPS[b] & 1), bool(FLIPS[b] & 2))
        assert torch.equal(got[b], want), f"image {b} {PARAMS[b]} flips {FLIPS[b]}: {(got[b] != want).sum().item()} values differ"
    unflipped = preprocess_images(torch.from_numpy(imgs).to(DEV), size, affine=mats).cpu()           # flips = None
    assert torch.equal(unflipped[1], reference_chain_affine(imgs[1], size, mats[1], False, False))


@pytest.mark.parametrize("order", [[1, 0, 2, 3], [0, 2, 3, 1]], ids=["contrast_first", "contrast_last"])
@pytest.mark.parametrize("src,size", [((33, 47), (96, 64)), ((160, 96), (64, 32)), ((160, 96), (70, 33))])
def test_affine_then_jitter_matches_pillow_bitwise(src, size, order):
    """The contrast op blends with the grey mean of the WARPED image, fill pixels included."""
    from structuredetector_amd.data import preprocess_images
    from structuredetector_amd.data.augment import jitter_words
    imgs, mats = _batch(src, size, seed=1)
    rng = np.random.default_rng(5)
    jits = [(order, float(rng.uniform(0.75, 1.25)), float(rng.uniform(0.75, 1.25)), float(rng.uniform(0.85, 1.15)), float(rng.uniform(-0.05, 0.05)))
            for _ in range(7)]
    words, factors = zip(*(jitter_words(*j) for j in jits))
    got = preprocess_images(torch.from_numpy(imgs).to(DEV), size, FLIPS, jitter=(list(words), list(factors)), affine=mats).cpu()
    for b in range(7):
        want = reference_chain_affine(imgs[b], size, mats[b], bool(FLIPS[b] & 1), bool(FLIPS[b] & 2), jits[b])
        assert torch.equal(got[b], want), f"image {b} {PARAMS[b]} {jits[b]}: {(got[b] != want).sum().item()} values differ"


def _random_jitter(rng, B):
    from structuredetector_amd.data.augment import jitter_words
    jit = [jitter_words(list(rng.permutation(4)), *rng.uniform(0.75, 1.25, 2), rng.uniform(0.85, 1.15), rng.uniform(-0.05, 0.05)) for _ in range(B)]
    return [w for w, _ in jit], [f for _, f in jit]


def test_identity_matrices_change_nothing():
    from structuredetector_amd.data import preprocess_images
    from structuredetector_amd.data.augment import affine_inverse_matrix
    rng = np.random.default_rng(9)
    imgs = torch.from_numpy(rng.integers(0, 256, (4, 75, 50, 3), dtype=np.uint8)).to(DEV)
    jitter = _random_jitter(rng, 4)
    for size in ((96, 64), (70, 33)):
        ident = [affine_inverse_matrix(size, 0, 1, (0, 0))] * 4
        assert ident[0] == [1, 0, 0, 0, 1, 0]
        for flips in (None, [0, 1, 2, 3]):
            assert torch.equal(preprocess_images(imgs, size, flips, affine=ident), preprocess_images(imgs, size, flips))
            assert torch.equal(preprocess_images(imgs, size, flips, jitter=jitter, affine=ident), preprocess_images(imgs, size, flips, jitter=jitter))
        assert torch.equal(preprocess_images(imgs, size, None, affine=np.asarray(ident)), preprocess_images(imgs, size))     # an array works too


def test_list_form_equals_the_packed_form():
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    from tests.test_gpu_image_cache import _arena_with
    rng = np.random.default_rng(21)
    hin, win = 37, 53
    imgs = [rng.integers(0, 256, (hin, win, 3), dtype=np.uint8) for _ in range(3)]
    arena, addrs = _arena_with(imgs, rng)
    assert all(a % 2 == 1 for a in addrs)
    order = [2, 0, 2, 1, 0, 1, 1]
    table = torch.tensor([addrs[t] for t in order], dtype=torch.int64, device=DEV)
    packed = torch.from_numpy(np.stack([imgs[t] for t in order])).to(DEV)
    jitter = _random_jitter(rng, 7)
    for size in ((96, 64), (70, 33)):
        _, mats = _batch((hin, win), size)
        for jit in (None, jitter):
            want = preprocess_images(packed, size, FLIPS, jitter=jit, affine=mats)
            got = preprocess_image_list(table, hin, win, size, FLIPS, jitter=jit, affine=mats)
            assert got.shape == (7, 3, size[1], size[0]) and torch.equal(got, want), (size, jit is not None)
    torch.cuda.synchronize()
    del arena


def test_fused_kernel_equals_the_u8_kernel_on_grey_images():
    """k_affine_norm (no jitter) against k_affine_u8 + the jitter stage with neutral parameters.  The jitter stage is NOT an exact
    pass-through on every colour (the HSV round trip of the hue op is not the identity: tests/test_gpu_pipeline.py), so on coloured images
    the two kernels are compared through the Pillow chain only (the tests above).  It IS exact where the hue op is: on grey pixels (the
    saturation-0 branch returns the value) and on the fill colour (124, 116, 104 survives Pillow's RGB -> HSV -> RGB); blends with factor 1
    return their input.  So on grey sources the two paths must agree bit for bit, fill included."""
    from structuredetector_amd.data import preprocess_images
    from structuredetector_amd.data.augment import jitter_words
    rng = np.random.default_rng(33)
    grey = np.repeat(rng.integers(0, 256, (7, 60, 80, 1), dtype=np.uint8), 3, axis=3)
    w, f = jitter_words([0, 1, 2, 3], 1.0, 1.0, 1.0, 0.0)
    for size in ((96, 64), (70, 33)):
        _, mats = _batch((60, 80), size)
        fused = preprocess_images(torch.from_numpy(grey).to(DEV), size, FLIPS, affine=mats)
        staged = preprocess_images(torch.from_numpy(grey).to(DEV), size, FLIPS, jitter=([w] * 7, [f] * 7), affine=mats)
        assert torch.equal(fused, staged), size
        fill = ((torch.tensor(FILL, dtype=torch.float32) / 255)[:, None, None] - MEAN) / STD
        assert (fused.cpu() == fill).all(1).any()                              # some pixels are fill: that ground is covered


def test_c_abi_rejects_bad_arguments_before_any_launch():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    B, Hin, Win, Hout, Wout = 2, 8, 8, 4, 4
    need = lib.sd_preprocess_affine_workspace_bytes(B, Hin, Win, Hout, Wout)
    m3, s3, fill = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25), (C.c_ubyte * 3)(*FILL)
    P = 4096                                                                   # never dereferenced: no call below reaches a launch
    for fn, name in ((lib.sd_preprocess_images_affine, b"sd_preprocess_images_affine"),
                     (lib.sd_preprocess_images_list_affine, b"sd_preprocess_images_list_affine")):
        def call(order=P, factors=P, affine=P, ws=need):
            return fn(P, B, Hin, Win, Hout, Wout, P, P, 3, P, P, 3, 0, order, factors, affine, fill, m3, s3, P, P, ws, 0)
        for what, kw, code in (("null affine", dict(affine=None), -1), ("order without factors", dict(factors=None), -1),
                               ("factors without order", dict(order=None), -1), ("workspace one byte short", dict(ws=need - 1), -2)):
            lib.sd_set_option(b"no_such_option", 1)                            # leaves another message behind
            assert call(**kw) == code, f"{name.decode()}: {what}"
            assert lib.sd_last_error() and name in lib.sd_last_error(), f"{name.decode()}: {what}: {lib.sd_last_error()}"


# ---- TrainAugmentation end to end -----------------------------------------------------------------------------------------------
SRC_H, SRC_W, OUT_W, OUT_H = 192, 256, 128, 96
# per image: objects of (anchor, parts) in SOURCE pixels (even: the 6 x 6 source blob becomes a 3 x 3 blob in the resized image)
LAYOUT = [((128, 96), [(60, 96), (128, 150)]), ((40, 40), [(90, 30), (20, 100)]), ((216, 160), [(170, 150), (236, 100)]),
          ((12, 180), [(60, 170)]), ((244, 12), [(200, 40)])]


def _scene():
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    img = np.zeros((SRC_H, SRC_W, 3), np.uint8)
    objects = []
    for k, (anchor, parts) in enumerate(LAYOUT):
        for x, y in (anchor, *parts):
            img[y - 2:y + 4, x - 2:x + 4] = 255                                  # pixels x - 2 .. x + 3: resized pixels x / 2 - 1 .. x / 2 + 1, centred on index x / 2
        objects.append(Object(f"o{k}", Keypoint("stem", float(anchor[0]), float(anchor[1])), [Keypoint(f"p{k}{j}", float(x), float(y))
                                                                                                   for j, (x, y) in enumerate(parts)]))
    return img, ImageAnnotation("s.png", objects)


def _peak_near(plane, x, y, radius=5):
    """Centre of the brightest plateau in the window around (x, y)."""
    H, W = plane.shape
    x0, x1, y0, y1 = max(int(round(x)) - radius, 0), min(int(round(x)) + radius + 1, W), max(int(round(y)) - radius, 0), min(int(round(y)) + radius + 1, H)
    win = plane[y0:y1, x0:x1]
    ys, xs = np.nonzero(win >= win.max() - 1e-6)
    return x0 + xs.mean(), y0 + ys.mean(), win.max()


def test_train_augmentation_moves_images_and_annotations_together():
    from structuredetector_amd.data import TrainAugmentation
    args = Namespace(width=OUT_W, height=OUT_H, no_augmentation=False, device=torch.device(DEV), aug_rotate=30.0, aug_scale=0.2, aug_translate=0.1)
    aug = TrainAugmentation(args)
    img, _ = _scene()
    torch.manual_seed(9)
    flips, _ = aug.draws_for(4)
    warps = aug.affine_draws_for(4)                                            # the draws the call below makes
    torch.manual_seed(9)
    out, anns = aug([img] * 4, [_scene()[1] for _ in range(4)])
    assert out.shape == (4, 3, OUT_H, OUT_W)
    out = out.cpu().numpy()
    dropped = kept = 0
    for i in range(4):
        angle, scale, tx, ty = warps[i]
        assert abs(angle) <= 30 and 0.8 <= scale <= 1.2 and abs(tx) <= 12.8 and abs(ty) <= 9.6
        c, s = np.cos(np.radians(angle)) * scale, np.sin(np.radians(angle)) * scale

        def where(x, y):                                                     # the host rule, written out: resize, warp about the centre, inside test
            u, v = x * OUT_W / SRC_W + 0.5 - OUT_W / 2, y * OUT_H / SRC_H + 0.5 - OUT_H / 2
            X, Y = c * u - s * v + OUT_W / 2 + tx, s * u + c * v + OUT_H / 2 + ty
            return (X - 0.5, Y - 0.5) if 0 <= X < OUT_W and 0 <= Y < OUT_H else None

        expect = {}
        for k, (anchor, parts) in enumerate(LAYOUT):
            if where(*anchor) is not None:
                expect[f"o{k}"] = [where(*anchor)] + [w for w in (where(*p) for p in parts) if w is not None]
                dropped += sum(where(*p) is None for p in parts)
            else:
                dropped += 1
        got = {o.name: [(o.x, o.y)] + [(p.x, p.y) for p in o.parts] for o in anns[i].objects}
        assert sorted(got) == sorted(expect) and all(len(got[n]) == len(expect[n]) for n in got), (i, got, expect)
        plane = out[i].sum(0)
        for n in got:
            for (gx, gy), (ex, ey) in zip(got[n], expect[n]):
                if flips[i] & 1:
                    ex = OUT_W - ex - 1
                if flips[i] & 2:
                    ey = OUT_H - ey - 1
                ex, ey = min(max(ex, 0), OUT_W - 1), min(max(ey, 0), OUT_H - 1)      # clip_annotation
                assert abs(gx - ex) <= 1e-9 and abs(gy - ey) <= 1e-9, (i, n)
                px, py, peak = _peak_near(plane, gx, gy)
                assert peak > plane.min() + 3.0 and np.hypot(px - gx, py - gy) <= 1.5, (i, n, (gx, gy), (px, py))
                kept += 1
    assert dropped >= 2 and kept >= 20, (dropped, kept)


def test_train_augmentation_with_the_flags_off_is_the_parent_path():
    from structuredetector_amd.data import TrainAugmentation, preprocess_images
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (60, 80, 3), dtype=np.uint8) for _ in range(4)]
    for extra in (dict(), dict(aug_rotate=0.0, aug_scale=0.0, aug_translate=0.0)):
        aug = TrainAugmentation(Namespace(width=128, height=96, no_augmentation=False, device=torch.device(DEV), **extra))
        torch.manual_seed(5)
        flips, jitter = aug.draws_for(4)
        state = torch.get_rng_state()
        want = preprocess_images(torch.from_numpy(np.stack(imgs)).to(DEV), (128, 96), flips, jitter=jitter)
        torch.manual_seed(5)
        got, anns = aug(imgs, [_scene()[1] for _ in range(4)])
        assert torch.equal(torch.get_rng_state(), state) and torch.equal(got, want)
        assert all(len(a.objects) == len(LAYOUT) for a in anns)                 # nothing is dropped without a warp
