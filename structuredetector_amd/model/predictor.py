"""Batched inference over a dataset: the loop behind `evaluate`, the trainer's validation pass and `detect`.

The reference walks its validation set ONE image at a time (src/sdnet/cli/evaluate.py:34-45, model/trainer.py:137-168,
cli/detect.py:28-41): PIL decode + Resize + ToTensor + Normalize on the host, upload, forward, Decoder, Evaluator -- each step
waiting for the one before.  Images are independent units (decode / evaluate are replicas only), so here

  * only the image DECODE stays on the host (threads, `data/feeder.BatchFeeder`: pinned staging, side-stream upload);
  * Resize + Normalize run for the whole batch on the GPU (`sd_preprocess_images`: Pillow's fixed-point bilinear resampling and
    torchvision's to_tensor / Normalize arithmetic, bit-identical bytes -- tests/test_gpu_pipeline.py);
  * forward + decoder run at `--eval_batch` images per launch, and batch n+1 is QUEUED before batch n's packed result is read
    (`Decoder.submit` / `PendingDecode.result`), so the host's object assembly and metric code overlap the GPU;
  * results come back per image, in dataset order: `Evaluator.accumulate` sees the same sequence as the reference's walk.

`Predictor` mirrors src/sdnet/model/predictor.py:8-37 (one PIL image in, one ImageAnnotation out).
"""
from __future__ import annotations

import torch


def index_batches(n, batch, lo=0):
    return [list(range(i, min(i + batch, n))) for i in range(lo, n, batch)]


def call_net(net, images, at_size):
    """`net(images)`; a wrapper that `needs_sources` (model/tta.py ScaleTta, model/tiles.py TiledNet: their other sizes are resampled from
    the source images) also gets `at_size`, a callable (width, height) -> the same images preprocessed at that size."""
    return net(images, at_size=at_size) if getattr(net, "needs_sources", False) else net(images)


def batched_decodes(net, decoder, dataset, args, batch=None, workers=None, with_raw_parts=True, depth=2, cache=None, index_range=None,
                    pr_curve=None):
    """dataset: `CropDataset(args, dir, raw=True)` or `PredictionDataset(dir, args, raw=True)` -- items ((H, W, 3) uint8 tensor,
    ImageAnnotation in ORIGINAL pixels with img_size).  Yields, per decoded batch and in dataset order,
    (list of prediction ImageAnnotations in network-input pixels, list of ground-truth annotations in network-input pixels (resized +
    clipped like Resize + Encode do, transforms.py:47-60,154), list of raw_parts or None, the batch's output dict of (B, C, h, w) views).
    index_range: (lo, hi), the items to run (a rank's shard, utils/distributed.shard_range); batches are cut inside it.  Default: all.
    cache: a data/image_cache.py DeviceImageCache the feed reads cached images from (CropDataset only), or None.
    pr_curve: a model/pr_curve.py PrCurve fed with every batch (queued right behind the decode, on its packed result when that holds the
    exact top-k; finished alongside the decode's result, so the queue-ahead overlap is kept), or None: nothing is launched."""
    from ..data.augment import ValidationAugmentation
    from ..data.feeder import BatchFeeder, default_decode_workers
    batch = int(batch or getattr(args, "eval_batch", 16) or 16)
    workers = workers or getattr(args, "decode_workers", 0) or default_decode_workers()
    lo, hi = index_range if index_range is not None else (0, len(dataset))
    if hi <= lo:                                   # an empty shard (more ranks than images)
        return
    prepare = ValidationAugmentation(args)
    pending = None

    def finish(p):
        handle, anns, out, matching = p
        preds, raws = handle.result()
        if matching is not None:
            matching.result()
        return list(preds), list(anns), (list(raws) if raws is not None else None), out

    threads = torch.get_num_threads()
    torch.set_num_threads(1)                       # the loop's host work is tiny tensor ops; torch's pool would spin against the decode threads
    try:
        for group in BatchFeeder(dataset, index_batches(hi, batch, lo), args.device, workers=workers, depth=depth, cache=cache):
            with torch.no_grad():
                images, anns = prepare(group, group.annotations)
                out = call_net(net, images, lambda size: prepare.images_at(group, size))
                if isinstance(out, torch.Tensor):  # Network(raw_output=True)
                    out = split_head(net, out)
                handle = decoder.submit(out, with_raw_parts=with_raw_parts)
                matching = None if pr_curve is None else pr_curve.submit(decoder, out, anns, packed=handle.packed if with_raw_parts else None)
            cur = (handle, anns, out, matching)
            if pending is not None:
                yield finish(pending)
            pending = cur
        if pending is not None:
            yield finish(pending)
    finally:
        torch.set_num_threads(threads)


def batched_outputs(net, decoder, dataset, args, batch=None, workers=None, with_raw_parts=True, keep_output=False, depth=2, cache=None,
                    index_range=None, pr_curve=None):
    """`batched_decodes` one image at a time: yields, per image and in dataset order, (prediction, ground-truth annotation, raw_parts or
    None, this image's output dict of (1, C, h, w) views when keep_output else None)."""
    for preds, anns, raws, out in batched_decodes(net, decoder, dataset, args, batch, workers, with_raw_parts, depth, cache, index_range,
                                                  pr_curve):
        for i, (pred, ann) in enumerate(zip(preds, anns)):
            yield pred, ann, (raws[i] if raws is not None else None), ({k: v[i:i + 1] for k, v in out.items()} if keep_output else None)


def split_head(net, out):
    """The four channel-slice views `Network.forward` returns (network.py:77-84) of a raw head tensor."""
    M, nb = net.label_count, net.label_count + net.part_count
    return {"anchor_hm": out[:, :M], "part_hm": out[:, M:nb], "offsets": out[:, nb:nb + 2], "embeddings": out[:, nb + 2:nb + 4]}


class Predictor(torch.nn.Module):
    """src/sdnet/model/predictor.py:8-37: network (weights from `args.pretrained_model`) + Decoder behind one call;
    `forward(image)` takes a PIL image (any size) and returns its ImageAnnotation in network-input pixels -- with `--keep_aspect` the
    pixels of the letterbox frame; `to_source(annotation, image.size)` maps either to the pixels of the image."""

    def __init__(self, args):
        super().__init__()
        from ..data import Decoder
        from .network import Network
        self.args = args
        from ..utils.args import check_keep_aspect
        self.keep_aspect = check_keep_aspect(args)                              # --keep_aspect: refused with --tiles / --tta_scales
        assert getattr(args, "pretrained_model", None), "No pretrained model specified. Use the option '--load_model <model_path>'."   # cli/evaluate.py:14-16
        self.model = Network(args, pretrained=False, init_weights=False)          # every tensor comes from the checkpoint (predictor.py:13-16)
        self.model.load_state_dict(torch.load(args.pretrained_model, map_location="cpu", weights_only=True), strict=True)
        self.model.eval().to(args.device)
        self.decoder = Decoder(args)
        self.tta = None
        if (getattr(args, "tta", "none") != "none" or getattr(args, "tta_scales", ()) or getattr(args, "tiles", ())
                or getattr(args, "tta_transpose", False) or getattr(args, "label_nms", 0)):     # --tta / --tta_scales: views, sizes + merged heatmaps (model/tta.py)
            from .tta import with_tta
            net, self.decoder = with_tta(self.model, self.decoder, args)
            self.tta = net if net is not self.model else None

    def forward(self, image):
        import numpy as np

        from ..data.augment import letterbox_geometry, preprocess_images
        arr = torch.from_numpy(np.asarray(image.convert("RGB"), np.uint8).copy())[None].to(self.args.device)
        size = (self.args.width, self.args.height)
        box = letterbox_geometry((arr.shape[2], arr.shape[1]), size) if self.keep_aspect else None
        with torch.no_grad():
            x = preprocess_images(arr, size, letterbox=box)
            return self.decoder(call_net(self.tta or self.model, x, lambda size: preprocess_images(arr, size)))[0]

    def to_source(self, annotation, image_size):
        """`forward`'s annotation (network-input pixels) in the pixels of the image it came from, image_size = (width, height) = PIL's
        `image.size`, in place: out of the letterbox frame with `--keep_aspect`, the plain rescale otherwise."""
        from ..utils.misc import unletterbox_annotation
        size = (self.args.width, self.args.height)
        if self.keep_aspect:
            return unletterbox_annotation(annotation, tuple(image_size), size)
        return annotation.resize(size, tuple(image_size))
