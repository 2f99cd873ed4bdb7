"""Command-line surface of the `train` / `evaluate` entry points.

Same flags, short options, dest names, defaults, validation and derived fields as the
reference's `Arguments` (src/sdnet/utils/args.py:17-269; table in SURVEY.md A.4), declared as a
table.  Extra (build-only) flags are grouped at the end and all default to "off".
"""
from __future__ import annotations

import argparse
import json
from collections import namedtuple
from multiprocessing import cpu_count
from pathlib import Path

import torch

from .misc import get_unique_color_map, set_seed

# (flags, kwargs)
_FLAGS = [
    (("--train_dir",), dict(type=str, help="The training directory.")),
    (("--valid_dir",), dict(type=str, help="The validation directory.")),
    (("--labels", "-m"), dict(type=str, default="labels.json", help="Json file of anchor and part names.")),
    (("--anchor_name", "-s"), dict(type=str, default="anchor", help="Name of the keypoint representing the anchor.")),
    (("--width", "-W"), dict(type=int, default=512, help="The network input width.")),
    (("--height", "-H"), dict(type=int, default=512, help="The network input height.")),
    (("--in_channels", "-c"), dict(type=int, default=3, help="Number of input channels.")),
    (("--fpn_depth",), dict(type=int, default=128, help="Depth of FPN layers of the decoder.")),
    (("--load_model", "-o"), dict(default=None, dest="pretrained_model", help="Load a previously trained model.")),
    (("--batch_size", "-b"), dict(type=int, default=8, help="Batch size for training.")),
    (("--epochs", "-e"), dict(type=int, default=100, help="The number of epochs to train.")),
    (("--no_augmentation", "-a"), dict(action="store_true", help="Disable training augmentations.")),
    (("--learning_rate", "-l"), dict(type=float, default=1e-3, help="The learning rate for training. The default is Adam's: "
                                     "--optimizer sgd usually wants a rate 10 to 100 times larger.")),
    (("--lr_step",), dict(type=int, default=3, help="Number of divisions by 10 of the learning rate (0 = off).")),
    (("--down_ratio", "-g"), dict(type=float, default=4.0, help="Downsampling ratio of the network.")),
    (("--hm_loss_fn", "-f"), dict(type=str, default="mse", help="Heatmap loss: 'focal' or 'mse'.")),
    (("--max_objects", "-n"), dict(type=int, default=20, help="Maximum number of objects per image.")),
    (("--max_parts", "-k"), dict(type=int, default=40, help="Maximum number of parts per image.")),
    (("--hm_weight",), dict(type=float, default=1.0, help="Weight for the heatmap loss.")),
    (("--offset_weight",), dict(type=float, default=0.001, help="Weight for the offset loss.")),
    (("--embedding_weight",), dict(type=float, default=0.001, help="Weight for the embedding loss.")),
    (("--sigma_gauss",), dict(type=float, default=10 / 100, help="Gaussian size, fraction of the image side.")),
    (("--conf_threshold", "-t"), dict(type=float, default=50 / 100, help="Confidence threshold in [0, 1].")),
    (("--dist_threshold", "-d"), dict(type=float, default=5 / 100, help="Evaluation radius, fraction of min side.")),
    (("--decoder_dist_thresh",), dict(type=float, default=10 / 100, help="Linkage radius, fraction of min side.")),
    (("--csi_threshold",), dict(type=float, default=75 / 100, help="Threshold on the CSI metric.")),
    (("--save_csv_eval",), dict(dest="csv_path", type=Path)),
    (("--amp",), dict(action="store_true", dest="use_amp", help="Automatic mixed precision.")),
    # build-only additions (data-parallel launcher / synthetic input)
    (("--synthetic",), dict(type=int, default=0, help="Train/evaluate on N seeded synthetic scenes instead of a directory.")),
    (("--steps",), dict(type=int, default=0, help="Stop training after this many optimizer steps (0 = full epochs).")),
    (("--bf16_inference",), dict(action="store_true", help="Eval-mode forward on the bf16 backbone (fp32 decode); training unaffected.")),
    (("--resume",), dict(type=str, default=None, help="Continue a run from trainings/<stamp>/resume.pth (weights, Adam state, scheduler, epoch).")),
    (("--decode_workers",), dict(type=int, default=0, help="Image decode threads of the directory feed (0 = half of this rank's CPU share, 2 .. 16).")),
    (("--prefetch",), dict(type=int, default=3, help="Batches decoded and uploaded ahead of the training step.")),
    (("--backbone_weights",), dict(type=str, default=None, help="torchvision ResNet-34 ImageNet state_dict (resnet34-b627a593.pth) for "
                                   "the trunk: what the reference downloads for pretrained=True (default: $SDNET_BACKBONE_WEIGHTS, then the torch hub cache).")),
    (("--log_dir",), dict(type=str, default=None, help="Directory for the training scalars (default: the run's save directory).")),
    (("--eval_batch",), dict(type=int, default=16, help="Images per forward + decode launch in evaluate / validation / detect.")),
    (("--sync_bn",), dict(action="store_true", help="Synchronized BatchNorm: data-parallel ranks normalise with the statistics of the "
                          "global batch (one fp64 all-reduce per BatchNorm and direction).")),
    (("--cache_images",), dict(type=float, default=0.0, help="GB of device memory for decoded training / validation images, kept across "
                               "epochs (decoded once before epoch 1; images beyond the budget are decoded every epoch; 0 = off).")),
    (("--weight_decay",), dict(type=float, default=0.0, help="Decoupled weight decay (torch.optim.AdamW) on the convolution weights; biases "
                               "and BatchNorm parameters are not decayed (0 = off: plain Adam). Under --optimizer sgd it is coupled L2 "
                               "(torch.optim.SGD: added to the gradient, so it passes through the momentum); under lamb it is added to the update.")),
    (("--clip_grad_norm",), dict(type=float, default=0.0, help="Clip the global norm of the (averaged) gradient to this value "
                                 "(torch.nn.utils.clip_grad_norm_); a step whose gradient norm is not finite is skipped -- this guard against inf / nan gradients (--amp) exists only with clipping on (0 = off).")),
    (("--ema_decay",), dict(type=float, default=0.0, help="Exponential moving average of the weights with this decay, warmed up as "
                            "min(decay, (1 + t) / (10 + t)); validation and model_best_*.pth use the average (0 = off).")),
    (("--tta",), dict(type=str, default="none", choices=["none", "hflip", "vflip", "hvflip"], help="Flip test-time augmentation in evaluate / "
                      "detect / Predictor: the network also runs on the mirrored image(s) (2 views for hflip and vflip, 4 for hvflip: the "
                      "forward sees that many times --eval_batch images), the heatmaps are averaged and decoded once. Not consulted by "
                      "train: its validation pass computes the loss from the plain head output.")),
    (("--tta_scales",), dict(type=str, default="", metavar="R[,R...]", help="Multi-scale test-time augmentation in evaluate / detect / "
                             "Predictor: comma-separated input-size ratios in [0.5, 2] (e.g. 0.75,1.25; the ratio 1 is implied). The network "
                             "also runs at int(R*W/32)*32 x int(R*H/32)*32 -- training's multi-scale rule, each size resampled from the source "
                             "image, at most 5 sizes -- the heatmaps are resampled to the base grid, averaged and decoded once. Combines "
                             "with --tta. Not consulted by train. Empty = off.")),
    (("--tta_transpose",), dict(action="store_true", help="Transposed-view test-time augmentation in evaluate / detect / Predictor: the "
                                "network also runs on the transposed image for every flip view, so the forward sees 2x the views (2 alone, "
                                "4 with --tta hflip or vflip, 8 with --tta hvflip: the eight symmetries of the grid; a non-square input takes "
                                "two forwards), the heatmaps are turned back, averaged and decoded once. Combines with --tta; does not "
                                "combine with --tta_scales / --tiles. Not consulted by train.")),
    (("--label_nms",), dict(type=int, default=0, metavar="R", help="Cross-label anchor suppression in evaluate / detect / Predictor: after "
                            "the per-label 5x5 NMS an anchor peak survives only where it equals the maximum over ALL label maps within R "
                            "output cells (1 .. 8), so an object that peaks under two labels at the same place or a cell apart is decoded "
                            "once, under the stronger label (the lower one on a tie). One max-pool, not a greedy loop; with R > 2 peaks of "
                            "one label closer than R are thinned too (the wider window for --tiles scale). Part maps are untouched. Combines "
                            "with --tta / --tta_scales / --tta_transpose / --tiles. Not consulted by train. 0 = off.")),
    (("--tiles",), dict(type=str, default="", metavar="CxR", help="Tiled inference in evaluate / detect / Predictor: columns x rows of "
                        "overlapping tiles (e.g. 2x2 or 3x2, each 1 .. 8). The source image is resized to a canvas of C*W - (C-1)*O by "
                        "R*H - (R-1)*O pixels (O = --tile_overlap), the network runs on every W x H tile -- the forward sees C*R times "
                        "--eval_batch images; --eval_batch keeps counting images -- and the tile heatmaps are stitched, blended over the "
                        "seams and decoded once. The canvas holds C*R times the area: raise --max_objects / --max_parts with it. Does not "
                        "combine with --tta / --tta_scales. Not consulted by train. Empty or 1x1 = off.")),
    (("--tile_overlap",), dict(type=int, default=64, metavar="PX", help="Pixels two neighbouring tiles of --tiles share: a multiple of 32 "
                               "in [0, min(W, H) / 2].")),
    (("--train_tiles",), dict(type=str, default="", metavar="CxR", help="Crop training at the scale of tiled inference: every training sample "
                              "is a W x H window, at a uniformly random position, of the source image resized to the canvas that --tiles CxR "
                              "with --tile_overlap would show the network (C*W - (C-1)*O by R*H - (R-1)*O pixels, following the per-epoch "
                              "multi-scale size); the other augmentations work on the window, objects whose anchor lies outside it are dropped. "
                              "Windows are drawn under --no_augmentation too. Needs a directory (not --synthetic). The validation pass of train "
                              "still shows whole frames: measure tiled deployment with evaluate --tiles. Not consulted by evaluate / detect. "
                              "Empty or 1x1 = off.")),
    (("--pr_curve",), dict(action="store_true", help="evaluate: also sweep the anchor-location and part-location metrics over the "
                           "confidence thresholds 0.01 .. 0.99 (and --conf_threshold) from ONE matching pass on the GPU, and print per "
                           "group the average precision (area under the precision envelope over recall), the best F1 with its threshold "
                           "and the operating point at --conf_threshold. CSI and classification stay at --conf_threshold. Only the "
                           "decoder's top-k slots are seen, which bounds the detections at low thresholds: raise --max_objects / "
                           "--max_parts. Not consulted by train / detect.")),
    (("--save_csv_pr",), dict(dest="csv_pr_path", type=Path, default=None, metavar="PATH", help="evaluate --pr_curve: write the curves here, "
                              "one row per group, label and threshold: tp, ndet, npos, precision, recall, F1, mean accuracy.")),
    (("--aug_rotate",), dict(metavar="DEG", help="Training augmentation: rotate every image about its centre by an "
                             "angle uniform in [-DEG, DEG] (0 .. 180; what leaves the frame is dropped from the annotation, what the image does "
                             "not cover is filled with the ImageNet mean; 0 = off). Not consulted by evaluate / detect.")),
    (("--aug_scale",), dict(metavar="S", help="Training augmentation: zoom every image about its centre by a factor "
                            "uniform in [1 - S, 1 + S] (0 <= S < 1; 0 = off). Not consulted by evaluate / detect.")),
    (("--aug_translate",), dict(metavar="T", help="Training augmentation: shift every image by a fraction of its width "
                                "and height uniform in [-T, T] (0 .. 0.5; 0 = off). Not consulted by evaluate / detect.")),
    (("--aug_mosaic",), dict(metavar="P", help="Training augmentation: with probability P (0 .. 1; 0 = off) an image "
                             "becomes a mosaic of itself and three other images of its batch at half scale around a random centre. A mosaic "
                             "carries up to four images' objects: raise --max_objects / --max_parts accordingly (what exceeds them is "
                             "truncated by the target encoder as always). Not consulted by evaluate / detect.")),
    (("--keep_aspect",), dict(action="store_true", help="Aspect-preserving network input in train (training and validation feeds) / evaluate / "
                              "detect / Predictor: the source image is resized, aspect ratio kept, to the largest size that fits "
                              "--width x --height and placed centred in a frame filled with the ImageNet mean (a letterbox), instead of "
                              "being stretched onto the frame; every augmentation and test-time view works on the frame; detect writes "
                              "original-image pixels. Train and evaluate a model with the same setting. Does not combine with --tiles / "
                              "--tta_scales / --train_tiles (their other sizes would letterbox with different roundings) or --synthetic. "
                              "Off = the stretched input.")),
    (("--aug_transpose",), dict(metavar="P", help="Training augmentation: with probability P (0 .. 1; 0 = off) an "
                                "image is transposed (x and y swapped: a lossless quarter turn with the flips, no resampling and no fill), "
                                "after the flips. Needs a square network input (--width equal to --height). Not consulted by evaluate / "
                                "detect.")),
    (("--aug_blur",), dict(metavar="R", help="Training augmentation: with the flip probability's threshold "
                           "(u < 0.5) an image is blurred by Pillow's GaussianBlur with a radius uniform in [0, R] pixels of the current "
                           "network input size (0 <= R <= 8: the same physical blur at every multi-scale size; motion / defocus blur of "
                           "deployment frames), after the warp and before the colour jitter; annotations are untouched. Needs a directory "
                           "(not --synthetic). Not consulted by evaluate / detect. 0 = off.")),
    (("--aug_perspective",), dict(metavar="D", help="Training augmentation: with the flip probability's threshold "
                                  "(u < 0.5) an image gets a random perspective warp, torchvision's RandomPerspective with distortion "
                                  "scale D (0 <= D <= 0.9): each corner of the frame moves inwards by up to D/2 of the width and height "
                                  "(pitch / roll / mounting tilt of the camera). Folded with --aug_rotate / --aug_scale / --aug_translate "
                                  "into one homography, so an image is resampled once, byte for byte Pillow's Image.transform("
                                  "PERSPECTIVE, BILINEAR); keypoints that leave the frame are dropped. Needs a directory (not "
                                  "--synthetic). Not consulted by evaluate / detect. 0 = off.")),
    (("--aug_jpeg",), dict(metavar="QMIN", help="Training augmentation: with the flip probability's threshold "
                           "(u < 0.5) an image is JPEG-compressed and decoded again at a quality uniform over the integers of [QMIN, 95] "
                           "(5 <= QMIN <= 95), byte for byte Pillow's save(quality=q) + open(): the 8 x 8 blocking, ringing and chroma "
                           "smearing of a camera's encoder, on the grid of the network input. After the blur and before the colour "
                           "jitter; annotations are untouched. Needs a directory (not --synthetic). Not consulted by evaluate / detect. "
                           "0 = off.")),
    (("--aug_equalize",), dict(metavar="P", help="Training augmentation: with probability P an image's histogram "
                               "is equalized per channel, byte for byte Pillow's ImageOps.equalize (torchvision's RandomEqualize on a PIL "
                               "image): a tone curve made from the image's own content, as exposure and auto-gain differences between "
                               "cameras are. After the JPEG round trip and before the colour jitter, on the 8-bit network input (fill "
                               "colour and letterbox bars included); annotations are untouched. Needs a directory (not --synthetic). Not "
                               "consulted by evaluate / detect. 0 = off.")),
    (("--aug_autocontrast",), dict(metavar="P", help="Training augmentation: with probability P an image that "
                                   "--aug_equalize did not select has each channel stretched to the full range, byte for byte Pillow's "
                                   "ImageOps.autocontrast (torchvision's RandomAutocontrast on a PIL image), ignoring a share of the "
                                   "darkest and brightest pixels uniform in [0, --aug_autocontrast_cutoff] percent. Same place in the chain "
                                   "and same limits as --aug_equalize. 0 = off.")),
    (("--aug_autocontrast_cutoff",), dict(metavar="C", help="Upper end, in percent of the pixels at either end of "
                                          "the histogram, of the cutoff that --aug_autocontrast draws (0 <= C <= 40).")),
    (("--aug_noise",), dict(metavar="R", help="Training augmentation: with probability 0.5 an image gets sensor read "
                            "noise, Gaussian with a standard deviation uniform in [0, R] grey levels (0 <= R <= 32), independent per pixel "
                            "and channel, as a camera at dusk or at short exposure delivers. Made on the GPU by a counter-based generator "
                            "(Philox4x32-10), bit-exact and reproducible from the seed. After the blur and before the JPEG round trip, on "
                            "the 8-bit network input (no gamma is modelled); annotations are untouched. Needs a directory (not "
                            "--synthetic). Not consulted by evaluate / detect. 0 = off.")),
    (("--aug_noise_shot",), dict(metavar="G", help="Training augmentation: the signal-dependent part of the sensor "
                                 "noise: a selected image's noise variance grows by g grey levels^2 per grey level, g uniform in [0, G] "
                                 "(0 <= G <= 2). Either of --aug_noise and --aug_noise_shot switches the stage on; same place in the chain "
                                 "and same limits. 0 = off.")),
    (("--freeze_stages",), dict(type=int, default=0, metavar="N", help="Fine-tuning: keep the first N trunk stages (stem, down1, down2, "
                                "down3, down4; 0 .. 5) as they were loaded: their convolution and BatchNorm parameters get no gradient and "
                                "never change, their BatchNorms normalise with the stored running statistics and do not update them "
                                "(Detectron2's FREEZE_AT). Their backward is not run. Not consulted by evaluate / detect. 0 = off.")),
    (("--freeze_bn",), dict(action="store_true", help="Fine-tuning: the BatchNorms of the trunk stages that still train use their stored "
                            "running statistics and keep their weight / bias (FrozenBatchNorm2d in the backbone); the convolutions around "
                            "them train, the three FPN BatchNorms keep batch statistics. Needs --freeze_stages >= 1. Not consulted by "
                            "evaluate / detect.")),
    (("--lr_schedule",), dict(type=str, default="step", choices=["step", "cosine"], help="Learning-rate schedule of train. step: the rate is "
                              "divided by 10 every epochs / --lr_step epochs (the reference's StepLR). cosine: it follows half a cosine "
                              "from --learning_rate to --min_lr over the optimizer steps of the run (epochs x steps per epoch, or --steps), "
                              "set before every step; --lr_step is then ignored. Not consulted by evaluate / detect.")),
    (("--warmup_steps",), dict(type=int, default=0, metavar="N", help="Linear warm-up, with either schedule: optimizer step i (from 0) of "
                               "the first N runs at (i + 1) / N of the scheduled rate (under cosine the cosine starts after the warm-up). "
                               "Must be less than the steps of the run. 0 = off.")),
    (("--min_lr",), dict(type=float, default=0.0, help="Rate at which --lr_schedule cosine ends (0 .. --learning_rate).")),
    (("--backbone_lr_mult",), dict(type=float, default=1.0, metavar="M", help="Fine-tuning: the pretrained trunk (stem, down1 .. down4) trains "
                                   "at M times the learning rate of the FPN and the head (0 .. 10; Detectron2 / MMDetection's backbone "
                                   "lr_mult), in the same single optimizer launch. A stage under --freeze_stages stays frozen. 1 = off.")),
    (("--lr_layer_decay",), dict(type=float, default=1.0, metavar="D", help="Fine-tuning: layer-wise learning-rate decay over the trunk: "
                                 "stage s (0 = stem .. 4 = down4) trains at M * D ** (5 - s) times the rate of the FPN and the head "
                                 "(0 < D <= 1; M = --backbone_lr_mult). 1 = off.")),
    (("--accum_steps",), dict(type=int, default=1, metavar="K", help="Gradient accumulation of train: one optimizer step uses the mean "
                              "gradient of K consecutive batches on each rank (1 .. 64), so the effective batch is K x --batch_size x ranks. "
                              "--steps, --warmup_steps, the cosine length and the EMA count optimizer steps, not batches. BatchNorm statistics "
                              "stay per batch (consider --freeze_bn or --sync_bn for small batches). Not consulted by evaluate / detect. "
                              "1 = off.")),
    (("--optimizer",), dict(type=str, default="adam", choices=["adam", "sgd", "lamb"], help="Update rule of train. adam: Adam / AdamW, as always. "
                            "sgd: torch.optim.SGD with --momentum (dampening 0; the usual fine-tuning optimizer). lamb: LAMB (You et al. 2020) -- "
                            "Adam's update scaled per convolution weight by |w| / |update|, for the large effective batches of --accum_steps and "
                            "many ranks; biases and BatchNorm parameters step without the ratio. Every other training flag works with all three; "
                            "a run resumes with the optimizer it was started with. Not consulted by evaluate / detect.")),
    (("--momentum",), dict(type=float, default=0.9, metavar="M", help="Momentum of --optimizer sgd, in [0, 1) (0 = plain SGD, no state buffer "
                           "is read or written); read by sgd only.")),
    (("--nesterov",), dict(action="store_true", help="Nesterov momentum for --optimizer sgd (needs --momentum > 0).")),
]

_POSITIVE = ["in_channels", "fpn_depth", "batch_size", "epochs", "learning_rate", "down_ratio", "max_objects", "max_parts"]
_NON_NEGATIVE = ["lr_step", "hm_weight", "offset_weight", "embedding_weight"]
_UNIT = ["conf_threshold", "dist_threshold", "decoder_dist_thresh", "csi_threshold"]


def _name_map(value):
    if isinstance(value, dict):
        return value
    if isinstance(value, list):
        return {name: i for i, name in enumerate(value)}
    return {value: 0}


def parse_tta_scales(text):
    """`--tta_scales`: "0.75,1.25" (or an already parsed sequence) -> the tuple of ratios, each in [0.5, 2]; "" -> ()."""
    if not isinstance(text, str):
        ratios = tuple(float(r) for r in text)
    else:
        try:
            ratios = tuple(float(t) for t in text.split(",")) if text.strip() else ()
        except ValueError:
            raise ValueError(f"'tta_scales' should be a comma-separated list of ratios (e.g. 0.75,1.25), not {text!r}") from None
    for r in ratios:
        if not 0.5 <= r <= 2:                       # (also false for nan)
            raise ValueError(f"'tta_scales' ratios should be in [0.5, 2], not {r}")
    return ratios


MAX_TILES = 8                       # tiles per axis (sd_tile_views / sd_tile_merge_nms)


def parse_tiles(text, name="tiles"):
    """`--tiles` (or `--train_tiles`: `name`): "3x2" (columns x rows; or an already parsed pair) -> (Tx, Ty), each in 1 .. 8; "" and "1x1" -> () (off)."""
    if not isinstance(text, str):
        grid = tuple(text)
        if len(grid) not in (0, 2) or any(int(v) != v for v in grid):
            raise ValueError(f"'{name}' should be COLUMNSxROWS (e.g. 2x2), not {text!r}")
        grid = tuple(int(v) for v in grid)
    else:
        fields = text.strip().lower().split("x") if text.strip() else []
        try:
            grid = tuple(int(f) for f in fields)
        except ValueError:
            grid = None
        if grid is None or len(grid) not in (0, 2):
            raise ValueError(f"'{name}' should be COLUMNSxROWS (e.g. 2x2), not {text!r}")
    for v in grid:
        if not 1 <= v <= MAX_TILES:
            raise ValueError(f"'{name}' should have 1 to {MAX_TILES} tiles per axis, not {v}")
    return () if grid == (1, 1) else grid


def check_tile_overlap(overlap, width, height):
    """`--tile_overlap` against the network input: a multiple of 32 in [0, min(W, H) / 2]; returns it as an int."""
    if int(overlap) != overlap or overlap % 32:
        raise ValueError(f"'tile_overlap' should be a multiple of 32, not {overlap}")
    if not 0 <= 2 * overlap <= min(width, height):
        raise ValueError(f"'tile_overlap' should be in [0, {min(width, height) // 2}] (half the smaller side of {width} x {height}), not {overlap}")
    return int(overlap)


def tile_canvas(width, height, grid, overlap):
    """(Wc, Hc) = (Tx*W - (Tx-1)*O, Ty*H - (Ty-1)*O): the canvas Tx x Ty tiles of W x H with overlap O cover."""
    tx, ty = grid
    return tx * width - (tx - 1) * overlap, ty * height - (ty - 1) * overlap


def tile_origins(width, height, grid, overlap):
    """The (row, column) pixel at which tile t = j*Tx + i starts: (j*(H-O), i*(W-O)), in t order."""
    tx, ty = grid
    return [(j * (height - overlap), i * (width - overlap)) for j in range(ty) for i in range(tx)]


def check_train_tiles(args):
    """`--train_tiles` on a parsed namespace -> (Tx, Ty) or () (off), as `train` checks it (model/trainer.py; `evaluate` and `detect` never
    look at the flag).  When it is on: `--synthetic` is refused (a rendered scene has no source
    image to cut a window from) and `--tile_overlap` must hold for the SMALLEST size the per-epoch multi-scale rule can produce,
    int(0.75 * side / 32) * 32 (the side itself under --no_augmentation): the canvas follows that size every epoch."""
    grid = parse_tiles(getattr(args, "train_tiles", ""), "train_tiles")
    if not grid:
        return grid
    if getattr(args, "synthetic", 0):
        raise ValueError("'train_tiles' cuts windows from source images: it needs --train_dir, not --synthetic")
    ratio = 1.0 if getattr(args, "no_augmentation", False) else 0.75
    width, height = int(ratio * args.width / 32) * 32, int(ratio * args.height / 32) * 32
    if min(width, height) < 32:
        raise ValueError(f"'train_tiles' needs a network input whose smallest multi-scale size is at least 32 x 32, not {width} x {height}")
    check_tile_overlap(getattr(args, "tile_overlap", 64), width, height)
    return grid


def check_keep_aspect(args, training=False):
    """`--keep_aspect` on a parsed namespace -> bool, as `train` (training=True), `evaluate`, `detect` and `Predictor` check it before any
    GPU work.  When it is on, the options whose other input sizes would letterbox with different integer roundings -- their grids would
    no longer align exactly -- are refused: `--train_tiles` by train, `--tiles` and `--tta_scales` by the others (train never consults
    those two); and `--synthetic`, which renders network-input tensors and has no source image to letterbox."""
    if not getattr(args, "keep_aspect", False):
        return False
    if training:
        if parse_tiles(getattr(args, "train_tiles", ""), "train_tiles"):
            raise ValueError("'keep_aspect' does not combine with --train_tiles: the canvas a window is cut from would letterbox with other "
                             "roundings than the frame; drop one of them")
    else:
        if parse_tiles(getattr(args, "tiles", "")):
            raise ValueError("'keep_aspect' does not combine with --tiles: the canvas would letterbox with other roundings than the frame and "
                             "the tile grids would not align; drop one of them")
        if parse_tta_scales(getattr(args, "tta_scales", "")):
            raise ValueError("'keep_aspect' does not combine with --tta_scales: every other input size would letterbox with its own roundings "
                             "and the heatmap grids would not align; drop one of them")
    if getattr(args, "synthetic", 0):
        raise ValueError("'keep_aspect' letterboxes source images: it needs a directory (--train_dir / --valid_dir), not --synthetic")
    return True


MAX_LABEL_NMS = 8                   # radius in cells (sd_label_nms / sd_nms5_labels)


def check_label_nms(radius):
    """`--label_nms`: an integer radius in output cells, 0 (off) .. 8; returns it as an int."""
    if isinstance(radius, bool) or int(radius) != radius:
        raise ValueError(f"'label_nms' should be an integer number of cells, not {radius!r}")
    if not 0 <= radius <= MAX_LABEL_NMS:
        raise ValueError(f"'label_nms' should be in [0, {MAX_LABEL_NMS}] (0 = off), not {radius}")
    return int(radius)


def check_aug_transpose(args):
    """`--aug_transpose` on a parsed namespace -> P, as `train` checks it (model/trainer.py): a batch has ONE shape, so a transposed sample
    needs width == height (the per-epoch multi-scale rule and the `--train_tiles` windows keep a square square)."""
    p = float(aug_flag(args, "aug_transpose"))
    if p > 0 and args.width != args.height:
        raise ValueError(f"'aug_transpose' transposes samples inside a batch of one shape: it needs a square network input, not "
                         f"{args.width} x {args.height}")
    return p


MAX_AUG_BLUR = 8.0                  # pixels: the gaussian radius whose box radius is SD_BLUR_MAX_RADIUS (include/sdnet_hip.h)
MAX_AUG_PERSPECTIVE = 0.9           # distortion scale: at 1 two opposite corners can meet and the quadrilateral degenerates
MIN_AUG_JPEG, MAX_AUG_JPEG = 5, 95  # qualities: below 5 every block is its mean, above 95 Pillow advises against (tables of ones)
MAX_AUG_AUTOCONTRAST_CUTOFF = 40.0  # percent at either end: beyond, the two cuts meet in the middle and most images are left alone
MAX_AUG_NOISE, MAX_AUG_NOISE_SHOT = 32.0, 2.0   # grey levels; levels^2 per level: where the stage clamps a row (2^26 and 2^17 in Q16)


# One training-augmentation flag: its default (what a Namespace from before the flag gives; the parser's default and type), its range
# [lo, hi] (open_hi: [lo, hi[; with lo > 0 the value 0 = off is accepted too), integer: an int is required, source: None or the verb of the
# refusal when the value is positive under --synthetic (the stage works on 8-bit source images and a rendered scene has none), text: what
# `check_aug` says the value should be, coerce: the value goes through float() instead of being refused when it is no number.
AugFlag = namedtuple("AugFlag", "name default lo hi open_hi integer source text coerce", defaults=(False, False, None, "in {range}", False))

# the table behind the parser's defaults, `finalize`'s asserts (in this order), `check_aug` and `TrainAugmentation`'s attributes (name[4:])
AUG_FLAGS = {f.name: f for f in (
    AugFlag("aug_rotate", 0.0, 0, 180),
    AugFlag("aug_scale", 0.0, 0, 1, open_hi=True),
    AugFlag("aug_translate", 0.0, 0, 0.5),
    AugFlag("aug_mosaic", 0.0, 0, 1),
    AugFlag("aug_transpose", 0.0, 0, 1),
    AugFlag("aug_blur", 0.0, 0, MAX_AUG_BLUR, source="blurs", text="in {range} pixels (0 = off)", coerce=True),
    AugFlag("aug_perspective", 0.0, 0, MAX_AUG_PERSPECTIVE, source="warps", text="in {range} (0 = off)", coerce=True),
    AugFlag("aug_jpeg", 0, MIN_AUG_JPEG, MAX_AUG_JPEG, integer=True, source="compresses", text="0 (off) or an integer in {range}"),
    AugFlag("aug_equalize", 0.0, 0, 1, source="work on", text="a probability in {range}"),
    AugFlag("aug_autocontrast", 0.0, 0, 1, source="work on", text="a probability in {range}"),
    AugFlag("aug_autocontrast_cutoff", 1.0, 0, MAX_AUG_AUTOCONTRAST_CUTOFF, text="a percentage in {range}"),
    AugFlag("aug_noise", 0.0, 0, MAX_AUG_NOISE, source="work on", text="in {range} grey levels (0 = off)"),
    AugFlag("aug_noise_shot", 0.0, 0, MAX_AUG_NOISE_SHOT, source="work on", text="in {range} (0 = off)"),
)}


def _aug_range(row):
    return f"[{row.lo:g}, {row.hi:g}{'[' if row.open_hi else ']'}"


def _aug_holds(row, v):
    """v lies in the row's range (false for nan)."""
    return bool(row.lo > 0 and v == 0) or (row.lo <= v < row.hi if row.open_hi else row.lo <= v <= row.hi)


def aug_flag(args, name):
    """The value of one flag of AUG_FLAGS on a namespace, unchecked: a namespace from before the flag gives its default; None, and for a
    flag whose default is 0 (= off) anything false, reads as 0."""
    row = AUG_FLAGS[name]
    v = getattr(args, name, row.default)
    return type(row.default)(0) if v is None or (not v and not row.default) else v


def check_aug(args, *names):
    """The flags `names` of AUG_FLAGS on a parsed namespace -> their values, as `train` checks them: each in its range and of its type (NaN
    fails the range test), then, under `--synthetic`, none of those that need source images positive."""
    rows = [AUG_FLAGS[n] for n in names]
    values = []
    for row in rows:
        v = aug_flag(args, row.name)
        if row.coerce:
            v = float(v)
        if isinstance(v, bool) or not isinstance(v, int if row.integer else (int, float)) or not _aug_holds(row, v):
            raise ValueError(f"'{row.name}' should be {row.text.format(range=_aug_range(row))}, not {v}")
        values.append(v if row.integer else float(v))
    needy = [row for row in rows if row.source]
    if getattr(args, "synthetic", 0) and any(v > 0 for row, v in zip(rows, values) if row.source):
        raise ValueError(f"{' / '.join(repr(row.name) for row in needy)} {needy[0].source} source images: "
                         f"{'it needs' if len(needy) == 1 else 'they need'} --train_dir, not --synthetic")
    return tuple(values)


# the checks of `train` by stage: the values in their ranges, a positive one refused with --synthetic (model/trainer.py calls `check_train`)
def check_aug_blur(args): return check_aug(args, "aug_blur")[0]                                  # noqa: E704  -> R, a radius in pixels
def check_aug_perspective(args): return check_aug(args, "aug_perspective")[0]                    # noqa: E704  -> D, a distortion scale
def check_aug_jpeg(args): return check_aug(args, "aug_jpeg")[0]                                  # noqa: E704  -> QMIN, 0 = off
def check_aug_tone(args): return check_aug(args, "aug_equalize", "aug_autocontrast", "aug_autocontrast_cutoff")   # noqa: E704  -> (P_eq, P_ac, C)
def check_aug_noise(args): return check_aug(args, "aug_noise", "aug_noise_shot")                 # noqa: E704  -> (R, G)


def check_train(args):
    """Everything `train` checks on a parsed namespace before it builds anything (model/trainer.py; `evaluate` and `detect` consult none of
    these flags): `--train_tiles`, `--keep_aspect`, `--aug_transpose`, then the ranges and the `--synthetic` refusals of AUG_FLAGS."""
    check_train_tiles(args)
    check_keep_aspect(args, training=True)
    for check in (check_aug_transpose, check_aug_blur, check_aug_perspective, check_aug_jpeg, check_aug_tone, check_aug_noise):
        check(args)


MAX_FREEZE_STAGES = 5               # stem, down1 .. down4 (model/network.py FREEZE_STAGES)


def check_freeze(args):
    """`--freeze_stages` / `--freeze_bn` on a parsed namespace -> (N, frozen BatchNorm), as `train` checks them (model/trainer.py;
    `evaluate`, `detect` and `Predictor` never look at the flags).  A namespace from before the flags gives (0, False).  N is an integer in
    0 .. 5; `--freeze_bn` needs N >= 1: with the stem frozen no trainable convolution sits in front of a frozen stem BatchNorm, whose
    backward (through the fused BatchNorm + ReLU + max-pool tail) is not built."""
    n, bn = getattr(args, "freeze_stages", 0), getattr(args, "freeze_bn", False)
    n = 0 if n is None else n
    if isinstance(n, bool) or not isinstance(n, int):
        raise ValueError(f"'freeze_stages' should be an integer number of trunk stages, not {n!r}")
    if not 0 <= n <= MAX_FREEZE_STAGES:
        raise ValueError(f"'freeze_stages' should be in [0, {MAX_FREEZE_STAGES}] (0 = off), not {n}")
    if bn and n == 0:
        raise ValueError("'freeze_bn' needs --freeze_stages >= 1: a frozen stem BatchNorm behind a trainable stem is not built")
    return n, bool(bn)


LrOptions = namedtuple("LrOptions", "schedule warmup_steps min_lr backbone_lr_mult lr_layer_decay")
LR_SCHEDULES = ("step", "cosine")
MAX_BACKBONE_LR_MULT = 10.0


def check_lr(args):
    """`--lr_schedule`, `--warmup_steps`, `--min_lr`, `--backbone_lr_mult`, `--lr_layer_decay` on a parsed namespace -> LrOptions, as
    `train` checks them (model/trainer.py; `evaluate`, `detect` and `Predictor` never look at the flags).  A namespace from before the
    flags gives the defaults (all off).  Every range test is false for NaN."""
    schedule = getattr(args, "lr_schedule", "step") or "step"
    if schedule not in LR_SCHEDULES:
        raise ValueError(f"'lr_schedule' should be one of {', '.join(LR_SCHEDULES)}, not {schedule!r}")
    n = getattr(args, "warmup_steps", 0)
    n = 0 if n is None else n
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"'warmup_steps' should be an integer number of optimizer steps >= 0, not {n!r}")
    base = float(getattr(args, "learning_rate", 1e-3))
    min_lr = float(getattr(args, "min_lr", 0.0) or 0.0)
    if not 0 <= min_lr <= base:
        raise ValueError(f"'min_lr' should be in [0, {base:g}] (0 to --learning_rate), not {min_lr}")
    mult = getattr(args, "backbone_lr_mult", 1.0)
    mult = 1.0 if mult is None else float(mult)
    if not 0 <= mult <= MAX_BACKBONE_LR_MULT:
        raise ValueError(f"'backbone_lr_mult' should be in [0, {MAX_BACKBONE_LR_MULT:g}] (1 = off), not {mult}")
    decay = getattr(args, "lr_layer_decay", 1.0)
    decay = 1.0 if decay is None else float(decay)
    if not 0 < decay <= 1:
        raise ValueError(f"'lr_layer_decay' should be in ]0, 1] (1 = off), not {decay}")
    return LrOptions(schedule, int(n), min_lr, mult, decay)


def stage_lr_mults(mult, decay):
    """{stage: multiplier} for `TrainStep(lr_mults=...)` from `--backbone_lr_mult` M and `--lr_layer_decay` D: trunk stage s (0 = stem ..
    4 = down4) gets M * D ** (5 - s), the FPN and the head 1; None when M = D = 1 (off: the step's launches are those without the flags)."""
    if mult == 1.0 and decay == 1.0:
        return None
    names = ("adpater", "down1", "down2", "down3", "down4")            # model/network.py FREEZE_STAGES
    return dict({name: mult * decay ** (5 - s) for s, name in enumerate(names)}, fpn=1.0, head=1.0)


MAX_ACCUM_STEPS = 64


def check_accum(args):
    """`--accum_steps` on a parsed namespace -> K, the batches per optimizer step, as `train` checks it (model/trainer.py; `evaluate`,
    `detect` and `Predictor` never look at the flag).  A namespace from before the flag gives 1 (off).  K is an integer in 1 .. 64."""
    k = getattr(args, "accum_steps", 1)
    k = 1 if k is None else k
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"'accum_steps' should be an integer number of batches per optimizer step, not {k!r}")
    if not 1 <= k <= MAX_ACCUM_STEPS:
        raise ValueError(f"'accum_steps' should be in [1, {MAX_ACCUM_STEPS}] (1 = off), not {k}")
    return k


OPTIMIZERS = ("adam", "sgd", "lamb")
OptimizerOptions = namedtuple("OptimizerOptions", "optimizer momentum nesterov")


def check_optimizer(args):
    """`--optimizer` / `--momentum` / `--nesterov` on a parsed namespace -> OptimizerOptions, as `train` checks them (model/trainer.py;
    `evaluate`, `detect` and `Predictor` never look at the flags).  A namespace from before the flags gives ("adam", 0.9, False).
    momentum is in [0, 1) (nan is refused) and is read by sgd only; nesterov under sgd needs momentum > 0."""
    kind = getattr(args, "optimizer", "adam")
    kind = "adam" if kind is None else kind
    if kind not in OPTIMIZERS:
        raise ValueError(f"'optimizer' should be one of {', '.join(OPTIMIZERS)}, not {kind!r}")
    momentum = getattr(args, "momentum", 0.9)
    momentum = 0.9 if momentum is None else momentum
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0 <= momentum < 1:       # (false for nan)
        raise ValueError(f"'momentum' should be in [0, 1), not {momentum!r}")
    nesterov = bool(getattr(args, "nesterov", False))
    if kind == "sgd" and nesterov and momentum == 0:
        raise ValueError("'nesterov' needs a 'momentum' greater than 0")
    return OptimizerOptions(kind, float(momentum), nesterov)


def updates_per_epoch(batches, accum_steps):
    """Optimizer steps of an epoch of `batches` batches under `--accum_steps K`: ceil(batches / K) -- the last group of an epoch is
    flushed with the batches it has (`TrainStep.flush`), so every epoch ends at an update boundary."""
    return -(-int(batches) // int(accum_steps))


def run_updates(epochs, batches, accum_steps=1, steps=0):
    """Optimizer steps of a whole run, the length of the cosine schedule: epochs x `updates_per_epoch`, or `--steps` (which counts
    optimizer steps too) when that is set and smaller."""
    total = int(epochs) * updates_per_epoch(batches, accum_steps)
    return min(total, int(steps)) if steps else total


def finalize(args):
    """Validation + derived fields (args.py:178-269) on an already parsed namespace."""
    for side in ("width", "height"):
        v = getattr(args, side)
        assert v % 32 == 0 and v > 0, f"{side.capitalize()} should be divisible by 32 and greater than 0"
    for k in _POSITIVE:
        assert getattr(args, k) > 0, f"'{k}' should be greater than 0"
    for k in _NON_NEGATIVE:
        assert getattr(args, k) >= 0, f"'{k}' should be greater than or equal to 0"
    for k in _UNIT:
        assert 0 <= getattr(args, k) <= 1, f"'{k}' should be in [0.0, 1.0]"
    assert 0 < args.sigma_gauss <= 1, "'sigma_gauss' should be in ]0.0, 1.0]"
    assert getattr(args, "cache_images", 0) >= 0, "'cache_images' should be greater than or equal to 0"
    for k in ("weight_decay", "clip_grad_norm", "ema_decay"):
        assert getattr(args, k, 0.0) >= 0, f"'{k}' should be greater than or equal to 0"
    assert getattr(args, "ema_decay", 0.0) < 1, "'ema_decay' should be less than 1"
    for row in AUG_FLAGS.values():
        assert _aug_holds(row, getattr(args, row.name, row.default)), f"'{row.name}' should be {'0 or ' if row.lo > 0 else ''}in {_aug_range(row)}"
    args.label_nms = check_label_nms(getattr(args, "label_nms", 0))
    args.tta_scales = parse_tta_scales(getattr(args, "tta_scales", ""))
    args.tiles = parse_tiles(getattr(args, "tiles", ""))
    args.tile_overlap = check_tile_overlap(getattr(args, "tile_overlap", 64), args.width, args.height) if args.tiles \
        else getattr(args, "tile_overlap", 64)
    args.train_tiles = parse_tiles(getattr(args, "train_tiles", ""), "train_tiles")      # checked by `train` (check_train_tiles); ignored by the others

    args.lr_step = int(args.epochs / args.lr_step) if args.lr_step != 0 else args.epochs
    for k in ("train_dir", "valid_dir", "pretrained_model"):
        if getattr(args, k, None) is not None:
            setattr(args, k, Path(getattr(args, k)).expanduser().resolve())

    if not isinstance(args.labels, dict):
        names = json.loads(Path(args.labels).expanduser().resolve().read_text())
        args.labels = _name_map(names["labels"])
        args.parts = _name_map(names["parts"])

    args.use_cuda = torch.cuda.is_available()          # ROCm PyTorch reports "cuda"
    if not args.use_cuda:
        raise RuntimeError("structuredetector_amd needs an MI355X visible as torch device 'cuda' (no CPU path)")
    args.device = torch.device("cuda", torch.cuda.current_device())
    args.num_workers = min(cpu_count(), 4)          # (args.py:251: the reference's DataLoader workers; the decode threads here: --decode_workers)
    set_seed(926354916)

    if args.hm_loss_fn.lower() not in {"focal", "mse"}:
        raise IOError(f"'hm_loss_fn' should either be 'focal' or 'mse', not {args.hm_loss_fn}.")
    args._r_labels = {v: k for k, v in args.labels.items()}
    args._r_parts = {v: k for k, v in args.parts.items()}
    args._label_color_map = get_unique_color_map(args.labels)          # args.py:264-267
    args._part_color_map = get_unique_color_map(args.parts)
    return args


class Arguments:
    def __init__(self):
        self.parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
        for flags, kw in _FLAGS:
            row = AUG_FLAGS.get(flags[0][2:])
            if row is not None:                                      # the augmentation flags take type and default from their table
                kw = dict(kw, type=type(row.default), default=row.default)
            self.parser.add_argument(*flags, **kw)

    def parse(self, argv=None):
        return finalize(self.parser.parse_args(argv))
