"""Aspect-preserving input on the GPU (sd_preprocess_images_letterbox / _list_letterbox: k_resample_h / k_resample_h_list at the inner
width, k_letterbox_v_norm, k_letterbox_v_u8) against Pillow itself -- Image.new(frame, FILL).paste(Image.resize(inner, BILINEAR)) ->
to_tensor -> Normalize, bit for bit --, against the existing entry points (exact fit; the later stages fed the Pillow frame), the
augmentation classes with `--keep_aspect` end to end, and `evaluate`, `detect`, `Predictor` and `train` with the flag."""
import functools
import json
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.letterbox_ref import (B, CASES, DIR_LABELS, DIR_PARTS, EXACT_FIT, FILL, FLIPS, flip_u8, geometry, normalize, pil_frame, sources,
                                 write_keep_aspect_dir)

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [f"{h}x{w}-{fw}x{fh}" for (h, w), (fw, fh), _ in CASES]


@functools.lru_cache(maxsize=None)
def _case(src, frame):
    """Images and the Pillow frames of one (source shape, frame): computed once, read only."""
    imgs = sources(src)
    frames = np.stack([pil_frame(imgs[b], frame) for b in range(B)])
    for a in (imgs, frames):
        a.setflags(write=False)
    return imgs, frames


def _arena(imgs, seed=1):
    from tests.test_gpu_image_cache import _arena_with
    arena, addrs = _arena_with(list(imgs), np.random.default_rng(seed))
    assert all(a % 2 == 1 for a in addrs)                                       # odd byte offsets inside one arena tensor
    return arena, torch.tensor(addrs, dtype=torch.int64, device=DEV)


def _box(src, frame):
    from structuredetector_amd.data import letterbox_geometry
    box = letterbox_geometry((src[1], src[0]), frame)
    assert box == geometry(src, frame)
    return box


@pytest.mark.parametrize("src,frame,_", CASES, ids=IDS)
def test_letterbox_matches_pillow_bitwise_packed_and_list(src, frame, _):
    """Normalize of Pillow's pasted resize is the reference, bytes and normalised values; nothing under test computes it."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    imgs, frames = _case(src, frame)
    box = _box(src, frame)
    x = torch.tensor(imgs, device=DEV)
    arena, table = _arena(imgs)
    mean, std = torch.tensor((0.485, 0.456, 0.406))[:, None, None], torch.tensor((0.229, 0.224, 0.225))[:, None, None]
    for flips in (None, FLIPS):
        packed = preprocess_images(x, frame, flips, letterbox=box).cpu()
        listed = preprocess_image_list(table, src[0], src[1], frame, flips, letterbox=box).cpu()
        assert packed.shape == listed.shape == (B, 3, frame[1], frame[0])
        for b in range(B):
            u8 = flip_u8(frames[b], flips[b] if flips else 0)
            want = normalize(u8)
            assert torch.equal(packed[b], want), f"packed: image {b} flips {flips}: {(packed[b] != want).sum().item()} values differ"
            assert torch.equal(listed[b], want), f"list: image {b} flips {flips}: {(listed[b] != want).sum().item()} values differ"
            # the bytes: un-normalising is exact to well under half a byte step, so rounding recovers them
            got_u8 = (packed[b] * std + mean).mul(255).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
            assert np.array_equal(got_u8, u8), f"bytes: image {b} flips {flips}"
    del arena
    wi, hi, px, py = box
    if (wi, hi) != tuple(frame):                                                # a bar pixel is the normalised fill byte, bit for bit
        bar = normalize(np.asarray(FILL, np.uint8).reshape(1, 1, 3))[:, 0, 0]
        y, xx = (0, 0) if (px or py) else (frame[1] - 1, frame[0] - 1)
        assert torch.equal(packed[0, :, y, xx], bar)


@pytest.mark.parametrize("src,frame,_", EXACT_FIT, ids=[IDS[CASES.index(c)] for c in EXACT_FIT])
def test_exact_fit_is_the_existing_entry_point_bit_for_bit(src, frame, _):
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    imgs, _frames = _case(src, frame)
    box = _box(src, frame)
    assert box == (frame[0], frame[1], 0, 0)
    x = torch.tensor(imgs, device=DEV)
    arena, table = _arena(imgs, seed=2)
    for name, kw in [("plain", {})] + _stage_sets(frame, B):
        want = preprocess_images(x, frame, **kw)
        want_list = preprocess_image_list(table, src[0], src[1], frame, **kw)
        assert torch.equal(want_list, want), name
        assert torch.equal(preprocess_images(x, frame, letterbox=box, **kw), want), name
        assert torch.equal(preprocess_image_list(table, src[0], src[1], frame, letterbox=box, **kw), want), name
    del arena


def _stage_sets(size, n):
    from tests.test_gpu_train_tiles import _jitter, _mosaic, _warps
    flips, jitter, warps, mosaic = FLIPS[:n], _jitter(n), _warps(size, n), _mosaic(size, n)
    return [("flips", dict(flips=flips)), ("jitter", dict(jitter=jitter)), ("affine", dict(affine=warps)), ("mosaic", dict(mosaic=mosaic)),
            ("jitter_flips", dict(flips=flips, jitter=jitter)), ("all", dict(flips=flips, jitter=jitter, affine=warps, mosaic=mosaic))]


@pytest.mark.parametrize("src,frame,_", [CASES[0], CASES[2], CASES[5]], ids=[IDS[0], IDS[2], IDS[5]])
def test_stages_on_a_letterbox_equal_the_existing_entry_points_on_the_pillow_frame(src, frame, _):
    """The later stages see the frame as they see a resized image: the existing entry points fed the Pillow frame bytes as (B, H, W, 3)
    sources at out_size = (W, H) -- an identity resize -- give the same tensor; the contrast mean is the frame's, bars included."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    imgs, frames = _case(src, frame)
    box = _box(src, frame)
    x, fx = torch.tensor(imgs, device=DEV), torch.tensor(frames, device=DEV)
    assert torch.equal(preprocess_images(fx, frame).cpu(), torch.stack([normalize(u) for u in frames]))     # the identity, checked
    arena, table = _arena(imgs, seed=7)
    for name, kw in _stage_sets(frame, B):
        want = preprocess_images(fx, frame, **kw)
        assert torch.equal(preprocess_images(x, frame, letterbox=box, **kw), want), name
        assert torch.equal(preprocess_image_list(table, src[0], src[1], frame, letterbox=box, **kw), want), name
    del arena


def test_a_letterbox_and_a_window_do_not_combine():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import preprocess_images
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.SdError, match="do not combine"):
        preprocess_images(x, (8, 8), letterbox=(8, 8, 0, 0), window=((8, 8), [(0, 0)]))
    with pytest.raises(L.SdError, match="does not lie inside"):                 # the library checks the geometry it is handed
        preprocess_images(x, (8, 8), letterbox=(8, 8, 1, 0))


# ---- the augmentation classes end to end -----------------------------------------------------------------------------------------
def _ann_rows(ann):
    return [(o.name, o.x, o.y, [(p.kind, p.x, p.y) for p in o.parts]) for o in ann.objects]


def _hand_composition(aug, raw, n, groups, keep):
    """What `aug(batch, annotations)` must give for the raw (image tensor, annotation) items, by replaying its draws (the caller seeded the
    generator) and composing by hand: Pillow frames, the existing entry points on them (an identity resize), and the host annotation rules
    in the chain's order.  keep=False: the stretched path as it was before the flag."""
    from structuredetector_amd.data import preprocess_images
    from structuredetector_amd.data.augment import _Objects, affine_forward_matrix, affine_inverse_matrix, mosaic_tiles
    from structuredetector_amd.utils.misc import affine_annotation, clip_annotation, hflip_annotation, mosaic_annotation, vflip_annotation
    W, H = aug.size
    flips, jitter = aug.draws_for(n)
    warps = aug.affine_draws_for(n)
    mosaics = aug.mosaic_draws_for(n, groups)
    out = torch.empty((n, 3, H, W))
    anns = [a.clone() for _, a in raw]
    for idx in groups:
        kw = {}
        if flips is not None:
            kw["flips"] = [flips[i] for i in idx]
            kw["jitter"] = ([jitter[0][i] for i in idx], [jitter[1][i] for i in idx])
        if warps is not None:
            kw["affine"] = [affine_inverse_matrix((W, H), a, s, (tx, ty)) for a, s, tx, ty in (warps[i] for i in idx)]
        if mosaics is not None:
            where = {i: k for k, i in enumerate(idx)}
            tiles = {i: mosaic_tiles((W, H), i, mosaics[i]) for i in idx}
            kw["mosaic"] = ([[*tiles[i][0][:2], *(where[s] for s in tiles[i][0][2:])] for i in idx], [tiles[i][1] for i in idx])
        if keep:
            stack = np.stack([pil_frame(raw[i][0].numpy(), (W, H)) for i in idx])
        else:
            stack = np.stack([raw[i][0].numpy() for i in idx])
        out[idx] = preprocess_images(torch.tensor(stack, device=DEV), (W, H), **kw).cpu()
        for i in idx:
            hin, win = raw[i][0].shape[:2]
            anns[i].img_size = anns[i].img_size or (win, hin)
            if keep:
                wi, hi, px, py = geometry((hin, win), (W, H))
                anns[i].resize((win, hin), (wi, hi))
                for o in anns[i].objects:
                    for kp in (o.anchor, *o.parts):
                        kp.x, kp.y = kp.x + px, kp.y + py
            else:
                anns[i].resize((win, hin), (W, H))
        if mosaics is not None:
            resized = {i: _Objects(anns[i].objects) for i in idx}
            for i in idx:
                if mosaics[i] is not None:
                    geom, _, forward, rects = tiles[i]
                    mosaic_annotation(anns[i], [resized[s] for s in geom[2:]], forward, rects)
        for i in idx:
            if warps is not None:
                a, s, tx, ty = warps[i]
                affine_annotation(anns[i], affine_forward_matrix((W, H), a, s, (tx, ty)), (W, H))
            if flips is not None and flips[i] & 1:
                hflip_annotation(anns[i], (W, H))
            if flips is not None and flips[i] & 2:
                vflip_annotation(anns[i], (W, H))
            clip_annotation(anns[i], (W, H))
    return out, anns


@pytest.mark.parametrize("extra", [dict(no_augmentation=True), dict(no_augmentation=False),
                                   dict(no_augmentation=False, aug_rotate=15.0, aug_scale=0.1, aug_mosaic=0.6)], ids=["letterbox", "jitter_flips", "all"])
def test_augmentations_with_keep_aspect_on_a_mixed_size_batch(golden_dir, tmp_path, extra):
    from structuredetector_amd.data import BatchFeeder, CropDataset, DeviceImageCache, ImageList, TrainAugmentation, ValidationAugmentation
    from tests.helpers import EVAL16_LABELS, EVAL16_PARTS, write_evaluate16_dir
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    common = dict(labels=EVAL16_LABELS, parts=EVAL16_PARTS, width=128, height=64, anchor_name="stem", device=torch.device(DEV, torch.cuda.current_device()))
    args = Namespace(keep_aspect=True, **common, **extra)
    ds = CropDataset(args, tmp_path / "train", raw=True)
    picks = [0, 1, 2, 3, 5, 8, 13, 4]
    raw = [ds[j] for j in picks]
    n = len(raw)
    batch = next(iter(BatchFeeder(ds, [picks], DEV, workers=2)))
    groups = [idx for idx, _ in batch.groups.values()]
    assert len(groups) > 1                                                      # several source sizes in the batch
    assert any(geometry(raw[i][0].shape[:2], (128, 64))[:2] != (128, 64) for i in range(n))     # and bars on some of them
    aug = TrainAugmentation(args)
    torch.manual_seed(31)
    want, want_anns = _hand_composition(aug, raw, n, groups, keep=True)
    state_on = torch.get_rng_state()
    torch.manual_seed(31)
    got, anns = aug(batch, [a.clone() for a in batch.annotations])
    assert torch.equal(torch.get_rng_state(), state_on)                         # the same draws, no more
    assert got.shape == (n, 3, 64, 128) and torch.equal(got.cpu(), want)
    assert [_ann_rows(a) for a in anns] == [_ann_rows(a) for a in want_anns]
    assert sum(len(a.objects) for a in anns) > 0
    if extra["no_augmentation"]:                                                # the rule written out: scale to the inner image, shift, clip
        for i, (img, ann) in enumerate(raw):
            (hin, win), (wi, hi, px, py) = img.shape[:2], geometry(img.shape[:2], (128, 64))
            assert len(anns[i].objects) == len(ann.objects)                     # nothing leaves the frame
            for o, q in zip(anns[i].objects, ann.objects):
                for kp, kq in zip((o.anchor, *o.parts), (q.anchor, *q.parts)):
                    assert abs(kp.x - min(max(kq.x * wi / win + px, 0), 127)) <= 1e-9 and abs(kp.y - min(max(kq.y * hi / hin + py, 0), 63)) <= 1e-9
        # validation is this chain without draws: the same tensor and annotations, and `images_at` the same tensor again
        val = ValidationAugmentation(args)
        state = torch.get_rng_state()
        v_got, v_anns = val(batch, [a.clone() for a in batch.annotations])
        assert torch.equal(torch.get_rng_state(), state)
        assert torch.equal(v_got, got) and [_ann_rows(a) for a in v_anns] == [_ann_rows(a) for a in anns]
        assert torch.equal(val.images_at(batch, (128, 64)), got)
    # the flag off: the draw sequence and the tensor of the stretched path, as before the flag
    off = TrainAugmentation(Namespace(**common, **extra))
    assert off.keep_aspect is False
    torch.manual_seed(31)
    off_want, off_want_anns = _hand_composition(off, raw, n, groups, keep=False)
    assert torch.equal(torch.get_rng_state(), state_on)                         # the flag draws nothing
    torch.manual_seed(31)
    off_got, off_anns = off(batch, [a.clone() for a in batch.annotations])
    assert torch.equal(torch.get_rng_state(), state_on) and torch.equal(off_got.cpu(), off_want)
    assert [_ann_rows(a) for a in off_anns] == [_ann_rows(a) for a in off_want_anns]
    assert not torch.equal(off_got, got)
    # the same batch through the device image cache: pointer tables instead of packed stacks, bit-identical
    cache = DeviceImageCache(1 << 28, DEV)
    cache.prefill(ds, workers=2)
    cached = next(iter(BatchFeeder(ds, [picks], DEV, workers=2, cache=cache)))
    assert all(isinstance(v, ImageList) for _, v in cached.groups.values())
    torch.manual_seed(31)
    got_cached, anns_cached = aug(cached, cached.annotations)
    assert torch.equal(got_cached, got) and [_ann_rows(a) for a in anns_cached] == [_ann_rows(a) for a in anns]


# ---- evaluate, detect, Predictor, train ------------------------------------------------------------------------------------------
SIZE = (128, 64)


@pytest.fixture()
def cli_setup(tmp_path, monkeypatch):
    from structuredetector_amd.model import Network
    monkeypatch.chdir(tmp_path)
    (tmp_path / "labels.json").write_text(json.dumps({"labels": list(DIR_LABELS), "parts": list(DIR_PARTS)}))
    torch.manual_seed(3)
    Network(Namespace(labels=DIR_LABELS, parts=DIR_PARTS, fpn_depth=128), pretrained=False).save(tmp_path / "w.pth")
    return tmp_path, ["-W", str(SIZE[0]), "-H", str(SIZE[1]), "-s", "stem", "--labels", str(tmp_path / "labels.json"), "-o", str(tmp_path / "w.pth"),
                      "-t", "0.05", "--keep_aspect"]


def _frames_batches(items, batch):
    """The normalised Pillow frames of the directory's images, in directory order, `batch` at a time."""
    frames = torch.stack([normalize(pil_frame(img, SIZE)) for img, _ in items]).to(DEV)
    return [frames[i:i + batch] for i in range(0, len(items), batch)]


def _ground_truth(items, directory):
    """The directory's annotations in frame pixels by hand: x * wi / win + px, then the clip."""
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    from structuredetector_amd.utils.misc import clip_annotation
    anns = []
    for n, (img, objs) in enumerate(items):
        (hin, win), (wi, hi, px, py) = img.shape[:2], geometry(img.shape[:2], SIZE)
        mv = lambda x, y: (x * (wi / win) + px, y * (hi / hin) + py)
        ann = ImageAnnotation(directory / f"img_{n}.png", [Object(l, Keypoint("stem", *mv(x, y)), [Keypoint(k, *mv(qx, qy)) for k, qx, qy in ps])
                                                            for l, x, y, ps in objs], img_size=(win, hin))
        anns.append(clip_annotation(ann, SIZE))
    return anns


@pytest.mark.parametrize("extra", [[], ["--tta", "hflip", "--label_nms", "2"]], ids=["plain", "hflip_label_nms"])
def test_evaluate_cli_with_keep_aspect_equals_the_hand_composition(cli_setup, extra):
    """Pillow frame -> Network -> Decoder -> Evaluator by hand (behind `with_tta` when the command line asks for views), batch for batch."""
    from structuredetector_amd.cli import evaluate
    from structuredetector_amd.data import Decoder
    from structuredetector_amd.model import Evaluator, Network
    from structuredetector_amd.model.tta import with_tta
    from structuredetector_amd.utils import Arguments
    from tests.test_gpu_label_nms_paths import evaluator_state
    tmp_path, common = cli_setup
    items = write_keep_aspect_dir(tmp_path / "valid")
    argv = common + ["--valid_dir", str(tmp_path / "valid"), "--eval_batch", "2"] + extra
    got = evaluate.main(argv)
    args = Arguments().parse(argv)
    net = Network(args, pretrained=False, init_weights=False)
    net.load_state_dict(torch.load(tmp_path / "w.pth", map_location="cpu", weights_only=True))
    net, decoder = with_tta(net.eval().to(args.device), Decoder(args), args)
    want = Evaluator(args)
    truth = _ground_truth(items, tmp_path / "valid")
    k = 0
    for frames in _frames_batches(items, 2):
        with torch.no_grad():
            preds, raws = decoder.submit(net(frames), with_raw_parts=True).result()
        for pred, raw in zip(preds, raws):
            want.accumulate(pred, truth[k], raw, True, True)
            k += 1
    assert k == len(items) and evaluator_state(got) == evaluator_state(want)
    assert got.anchor_eval.reduce().npos == 3 * len(items) and got.anchor_eval.reduce().ndet > 0
    # and the flag matters: the stretched input gives another result on these non-square images
    plain = evaluate.main([a for a in argv if a != "--keep_aspect"])
    assert evaluator_state(plain) != evaluator_state(got)


def _predict_by_hand(args, weights, items, batch):
    from structuredetector_amd.data import Decoder
    from structuredetector_amd.model import Network
    net = Network(args, pretrained=False, init_weights=False)
    net.load_state_dict(torch.load(weights, map_location="cpu", weights_only=True))
    net, decoder = net.eval().to(args.device), Decoder(args)
    preds = []
    for frames in _frames_batches(items, batch):
        with torch.no_grad():
            preds += list(decoder.submit(net(frames), with_raw_parts=False).result()[0])
    return preds


def test_detect_cli_and_predictor_with_keep_aspect_return_original_pixels(cli_setup):
    from PIL import Image
    from structuredetector_amd.cli import detect
    from structuredetector_amd.model.predictor import Predictor
    from structuredetector_amd.utils import Arguments
    from structuredetector_amd.utils.misc import unletterbox_annotation
    from tests.test_gpu_tta import ann_key
    tmp_path, common = cli_setup
    items = write_keep_aspect_dir(tmp_path / "imgs", jpg=True)
    written = detect.main(common + ["--valid_dir", str(tmp_path / "imgs"), "--eval_batch", "2"])
    assert [p.name for p in written] == [f"img_{n}.json" for n in range(len(items))]
    args = Arguments().parse(common)
    preds = _predict_by_hand(args, tmp_path / "w.pth", items, 2)
    assert sum(len(p.objects) for p in preds) > 0
    predictor = Predictor(args)
    assert predictor.keep_aspect is True
    for n, ((img, _), pred, path) in enumerate(zip(items, preds, written)):
        hin, win = img.shape[:2]
        wi, hi, px, py = geometry((hin, win), SIZE)
        js = json.loads(path.read_text())
        assert js["img_size"] == [win, hin]
        got = [(o["label"], [(p["kind"], p["location"]["x"], p["location"]["y"]) for p in o["parts"]]) for o in js["objects"]]
        want = [(o.name, [(kp.kind, (kp.x - px) * (win / wi), (kp.y - py) * (hin / hi)) for kp in (o.anchor, *o.parts)]) for o in pred.objects]
        assert got == want, n                                                   # the way back written out: out of the frame, then the scale
        # Predictor: frame pixels from forward (one image per call: its own batch of one), the same original pixels through to_source
        image = Image.open(tmp_path / "imgs" / f"img_{n}.jpg")
        one = _predict_by_hand(args, tmp_path / "w.pth", [items[n]], 1)[0]
        ann = predictor(image)
        assert ann_key(ann) == ann_key(one)
        back = unletterbox_annotation(one.clone(), (win, hin), SIZE)
        assert ann_key(predictor.to_source(ann, image.size)) == ann_key(back)
    # without the flag `to_source` is the plain rescale
    plain = Predictor(Arguments().parse([a for a in common if a != "--keep_aspect"]))
    image = Image.open(tmp_path / "imgs" / "img_1.jpg")
    ann = plain(image)
    want = ann.clone().resize(SIZE, image.size)
    assert plain.keep_aspect is False and ann_key(plain.to_source(ann, image.size)) == ann_key(want)


def test_train_cli_with_keep_aspect_trains_and_validates_on_letterboxed_frames(cli_setup, monkeypatch, capsys):
    """Two steps of `train --keep_aspect` and the validation pass of epoch 0: the training feed hands out frames of the network input's
    shape with the flag read, and the validation forward sees exactly the normalised Pillow frames of the validation directory."""
    import re

    from structuredetector_amd.cli import train
    from structuredetector_amd.data import augment as A
    from structuredetector_amd.model import predictor as P
    tmp_path, common = cli_setup
    write_keep_aspect_dir(tmp_path / "train")
    items = write_keep_aspect_dir(tmp_path / "valid")
    seen, fed = [], []
    call_net, prepare = P.call_net, A.ValidationAugmentation.__call__

    def spy(net, images, at_size):
        seen.append(images.detach().cpu())
        return call_net(net, images, at_size)

    def record(aug, images, annotations):
        out = prepare(aug, images, annotations)
        fed.append((type(aug).__name__, tuple(out[0].shape[1:]), aug.keep_aspect))
        return out
    monkeypatch.setattr(P, "call_net", spy)
    monkeypatch.setattr(A.ValidationAugmentation, "__call__", record)
    argv = [a for a in common if a not in ("-o", str(tmp_path / "w.pth"))]
    torch.manual_seed(1)
    train.main(argv + ["--train_dir", str(tmp_path / "train"), "--valid_dir", str(tmp_path / "valid"), "-b", "2", "-e", "1", "--steps", "2",
                       "--decode_workers", "2", "--eval_batch", "5", "--no_augmentation"])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("epoch 0:")]
    assert len(line) == 1 and "(2 steps)" in line[0], out
    losses = [float(v) for v in re.findall(r"(?:total|hm|offset|embedding) (\S+)", line[0])]
    assert len(losses) == 4 and np.isfinite(losses).all() and losses[0] > 0
    assert [f for f in fed if f[0] == "TrainAugmentation"] == [("TrainAugmentation", (3, SIZE[1], SIZE[0]), True)] * 2
    assert [f for f in fed if f[0] == "ValidationAugmentation"] == [("ValidationAugmentation", (3, SIZE[1], SIZE[0]), True)]
    assert "validation (5 images)" in out and len(seen) == 1                    # the validation pass: one batch of five letterboxed frames
    assert torch.equal(seen[0], torch.stack([normalize(pil_frame(img, SIZE)) for img, _ in items]))
