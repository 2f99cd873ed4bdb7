from .dataset import CropDataset, PredictionDataset, collate_fn
from .decoders import Decoder, FusedOutputDecoder, RawDecoder, TiledOutputDecoder
from .transforms import Encode
from .augment import (TrainAugmentation, ValidationAugmentation, affine_forward_matrix, affine_inverse_matrix, blur_box_params, blur_images,
                      compose_affine_perspective, jpeg_images, jpeg_quant_tables, jpeg_rows, letterbox_geometry, mosaic_tiles, noise_images, noise_rows, perspective_coeffs, perspective_images, pil_bilinear_coeffs,
                      preprocess_image_list, preprocess_images, tone_images, tone_rows, window_extents)
from .feeder import BatchFeeder, GroupedBatch
from .image_cache import DeviceImageCache, ImageList
