"""The windowed resize on the host, for tests/test_train_tiles_cpu.py and tests/test_gpu_train_tiles.py: image b's window is
`Image.fromarray(src).resize((Wc, Hc), BILINEAR).crop((x0, y0, x0 + w, y0 + h))`, computed by Pillow itself; `CASES` are the shapes the
tests share."""
import numpy as np

MEAN3 = (0.485, 0.456, 0.406)
STD3 = (0.229, 0.224, 0.225)

# ((Hin, Win) source, (w, h) window, (Tx, Ty) grid, overlap): a downscale, an upscale, the identity, and an anisotropic 128 x 64 canvas
CASES = [((150, 201), (64, 64), (2, 2), 32), ((40, 50), (64, 64), (2, 2), 32), ((96, 96), (64, 64), (2, 2), 32), ((61, 333), (64, 48), (3, 2), 32)]
# canvases no grid gives, handed to the window argument directly: (61, 333) -> 160 x 96 (the anisotropic shape checked on the CPU)
FREE_CASES = [((61, 333), (64, 48), (160, 96))]
B = 5


def canvas_of(size, grid, overlap):
    (w, h), (tx, ty) = size, grid
    return tx * w - (tx - 1) * overlap, ty * h - (ty - 1) * overlap


def origins5(canvas, size):
    """The four corner origins and one odd interior origin."""
    (Wc, Hc), (w, h) = canvas, size
    mx, my = Wc - w, Hc - h
    return [(0, 0), (mx, 0), (0, my), (mx, my), (min(mx, (mx // 2) | 1), min(my, (my // 2) | 1))]


def sources(shape, n=B, seed=None):
    rng = np.random.default_rng(shape[0] * 1009 + shape[1] if seed is None else seed)
    return rng.integers(0, 256, (n, shape[0], shape[1], 3), dtype=np.uint8)


def pil_window(src, canvas, origin, size):
    """(h, w, 3) uint8: the crop of Pillow's resize of one (Hin, Win, 3) uint8 image."""
    from PIL import Image
    (x0, y0), (w, h) = origin, size
    return np.asarray(Image.fromarray(src).resize(tuple(canvas), Image.BILINEAR).crop((x0, y0, x0 + w, y0 + h))).copy()


def normalize(u8):
    """to_tensor + Normalize of an (h, w, 3) uint8 image: (3, h, w) fp32, two correctly rounded fp32 operations each."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).to(torch.float32).div(255)
    return t.sub(torch.tensor(MEAN3)[:, None, None]).div(torch.tensor(STD3)[:, None, None])


def brute_extent(in_size, canvas_size, out_size):
    """The largest source span of any window along one axis, by trying every origin on `pil_bilinear_coeffs`' table."""
    from structuredetector_amd.data.augment import pil_bilinear_coeffs
    bounds = pil_bilinear_coeffs(in_size, canvas_size)[0]
    best = 0
    for o in range(canvas_size - out_size + 1):
        lo = int(bounds[o, 0])
        hi = int(bounds[o + out_size - 1, 0] + bounds[o + out_size - 1, 1])
        best = max(best, hi - lo)
    return best
