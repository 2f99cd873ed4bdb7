"""The letterbox (`--keep_aspect`) on the host, for tests/test_letterbox_cpu.py and tests/test_gpu_letterbox.py: image b's frame is
`Image.new("RGB", (W, H), FILL)` with `Image.fromarray(src).resize((wi, hi), BILINEAR)` pasted at (px, py), computed by Pillow itself;
`CASES` are the shapes the tests share and `write_keep_aspect_dir` the PNG + JSON directory of non-square images the CLI tests read."""
import numpy as np

from tests.window_ref import MEAN3, STD3, normalize, sources  # noqa: F401  (normalize / sources: what the window tests use)

FILL = (124, 116, 104)                                        # the ImageNet mean in bytes (data/augment.py _FILL)

# ((Hin, Win) source, (W, H) frame, (wi, hi, px, py) from the issue's table where it lists the case, what it covers)
CASES = [
    ((37, 23), (64, 32), (20, 32, 22, 0)),          # portrait, side bars, odd sizes
    ((23, 37), (64, 32), None),                     # landscape, side bars
    ((204, 245), (64, 64), (64, 53, 0, 5)),         # downscale, odd bar split 5 / 6
    ((20, 30), (96, 64), None),                     # upscale, exact fit
    ((1, 300), (64, 64), (64, 1, 0, 31)),           # one inner row
    ((300, 1), (64, 32), None),                     # one inner column
    ((48, 96), (64, 32), (64, 32, 0, 0)),           # same aspect, no bars
]
EXACT_FIT = [c for c in CASES if c[0] in ((20, 30), (48, 96))]
B = 5
FLIPS = [0, 1, 2, 3, 1]


def geometry(src, frame):
    """The issue's rule, restated with its own integers (not imported from the code under test)."""
    (hin, win), (W, H) = src, frame
    if W * hin <= H * win:
        wi, hi = W, min(H, max(1, (hin * W + win // 2) // win))
    else:
        hi, wi = H, min(W, max(1, (win * H + hin // 2) // hin))
    return wi, hi, (W - wi) // 2, (H - hi) // 2


def pil_frame(src, frame, fill=FILL):
    """(H, W, 3) uint8: Pillow's letterbox of one (Hin, Win, 3) uint8 image."""
    from PIL import Image
    wi, hi, px, py = geometry(src.shape[:2], frame)
    f = Image.new("RGB", tuple(frame), tuple(fill))
    f.paste(Image.fromarray(src).resize((wi, hi), Image.BILINEAR), (px, py))
    return np.asarray(f).copy()


def flip_u8(u8, f):
    """The flips of the pipeline on an (H, W, 3) image: bit 0 horizontal, bit 1 vertical."""
    if f & 1:
        u8 = u8[:, ::-1]
    if f & 2:
        u8 = u8[::-1]
    return np.ascontiguousarray(u8)


# image sizes (width, height) of the CLI directory: landscape, portrait, wide, the frame's own aspect (no bars at 128 x 64), and a repeat so
# that one size group holds two images
DIR_SIZES = [(160, 112), (96, 144), (224, 64), (192, 96), (160, 112)]
DIR_LABELS = {"bean": 0, "maize": 1}
DIR_PARTS = {"leaf": 0}


def write_keep_aspect_dir(directory, jpg=False):
    """img_N.png + img_N.json (README schema, "box": null) of blocky seeded noise, three objects with one or two parts each, all inside the
    image; with jpg=True only img_N.jpg (what `detect` reads).  Returns [(uint8 array, [(label, x, y, [(kind, px, py)])])]."""
    import json
    from pathlib import Path

    from PIL import Image
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    items = []
    for n, (iw, ih) in enumerate(DIR_SIZES):
        rng = np.random.default_rng(500 + n)
        small = rng.integers(0, 256, (ih // 16, iw // 16, 3), dtype=np.uint8)
        img = np.repeat(np.repeat(small, 16, 0), 16, 1)
        objs = []
        for k in range(3):
            x, y = float(rng.integers(8, iw - 8)), float(rng.integers(8, ih - 8))
            parts = [("leaf", float(min(max(x + dx, 0), iw - 1)), float(min(max(y + dy, 0), ih - 1)))
                     for dx, dy in rng.integers(-12, 13, (1 + k % 2, 2)).tolist()]
            objs.append((("bean", "maize")[k % 2], x, y, parts))
        if jpg:
            Image.fromarray(img).save(directory / f"img_{n}.jpg", quality=95)
            img = np.asarray(Image.open(directory / f"img_{n}.jpg").convert("RGB")).copy()
        else:
            Image.fromarray(img).save(directory / f"img_{n}.png")
            js = {"image_path": str(directory / f"img_{n}.png"), "img_size": [iw, ih],
                  "objects": [{"label": l, "box": None, "parts": [{"kind": "stem", "location": {"x": x, "y": y}}]
                               + [{"kind": k, "location": {"x": px, "y": py}} for k, px, py in ps]} for l, x, y, ps in objs]}
            (directory / f"img_{n}.json").write_text(json.dumps(js))
        items.append((img, objs))
    return items
