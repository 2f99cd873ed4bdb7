"""`detect` entry point (reference: src/sdnet/cli/detect.py:13-53): run the network + decoder over every `.jpg` of
`--valid_dir`, write `predictions/<name>.json` (annotation in original image pixels) and the image with the objects drawn.
Images are decoded by threads and go through Resize + Normalize, forward and decoder in batches of `--eval_batch`
(model/predictor.py); outputs are written per image in the directory's order, like the reference's walk.

Multi-GPU (`python -m torch.distributed.run --nproc-per-node N -m structuredetector_amd.cli.detect ...`): each rank writes the files
of its contiguous shard of the directory only; the written lists are gathered in rank order, so `main()` returns the whole list in
directory order on every rank."""
from pathlib import Path

import torch
import torch.distributed as dist
from PIL import Image

from ..data import Decoder
from ..data.dataset import PredictionDataset
from ..model import Network
from ..utils import Arguments, draw
from ..utils.args import check_keep_aspect
from ..utils.misc import unletterbox_annotation
from ..utils.distributed import gather_objects, init_from_env, shard_range, world_info


def main(argv=None):
    created = init_from_env()
    try:
        return _detect(argv)
    finally:
        if created:
            dist.destroy_process_group()


def _detect(argv):
    args = Arguments().parse(argv)
    assert args.valid_dir, "Path to a directory with the images to process must be specified (--valid_dir)."
    keep_aspect = check_keep_aspect(args)                  # --keep_aspect: refused with --tiles / --tta_scales
    rank, world = world_info()
    dataset = PredictionDataset(args.valid_dir, args, raw=True)
    decoder = Decoder(args)
    net = Network(args, pretrained=not args.pretrained_model, init_weights=not args.pretrained_model)             # detect.py:24-25: every tensor comes from the checkpoint
    if args.pretrained_model:
        net.load_state_dict(torch.load(args.pretrained_model, map_location="cpu", weights_only=True))
    net = net.eval().to(args.device)
    if (getattr(args, "tta", "none") != "none" or getattr(args, "tta_scales", ()) or getattr(args, "tiles", ())
            or getattr(args, "tta_transpose", False) or getattr(args, "label_nms", 0)):
        from ..model.tta import with_tta
        net, decoder = with_tta(net, decoder, args)
    out_dir = Path("predictions")
    out_dir.mkdir(exist_ok=True)
    written = []
    from ..model.predictor import batched_outputs
    shard = shard_range(len(dataset), rank, world)
    for annotation, source, _, _ in batched_outputs(net, decoder, dataset, args, with_raw_parts=False, index_range=shard):
        img_size, image_path = source.img_size, source.image_path
        if keep_aspect:                                                 # back to the pixels of the original image: out of the frame, then the scale
            unletterbox_annotation(annotation, img_size, (args.width, args.height))
        else:
            annotation.resize((args.width, args.height), img_size)
        annotation.img_size = img_size
        annotation.image_path = image_path
        image = draw(Image.open(image_path).convert("RGB"), annotation, args)
        annotation.save_json(out_dir)
        image.save(out_dir / image_path.name)
        written.append(out_dir / image_path.with_suffix(".json").name)
    return gather_objects(written)


detect = main

if __name__ == "__main__":
    main()
