"""`preprocess_images` / `preprocess_image_list` (one sd_preprocess_chain call each) against the legacy entry points of the C API called by
name with positional arguments (tests/helpers.py call_legacy_preprocess_form), bit for bit: every geometry x stage set x late set of
tests/test_preprocess_plan_cpu.py, packed and list, plus a batch of one, the smallest JPEG frame and an odd frame.  What the legacy forms
compute is pinned to Pillow by the tests of their stages; this file proves that the chain and every legacy wrapper fill the one descriptor
alike."""
import numpy as np
import pytest
import torch

from tests.test_gpu_blur import OUT, SRC, _geometry, _sources, _stage_sets, _table

pytestmark = pytest.mark.gpu
DEV = "cuda"
LATE_SETS = [(), ("blur",), ("persp",), ("noise",), ("jpeg",), ("tone",), ("persp", "blur", "noise", "jpeg", "tone")]
LEGACY_ORDER = ["noise", "tone", "jpeg", "persp", "blur", "letterbox", "window", "mosaic", "affine", "jitter"]       # highest form first


def _late_tables(size, n):
    """One table per late stage for n images at size = (width, height); row 0 of blur, noise, jpeg and tone leaves its image as it is."""
    from structuredetector_amd.data import blur_box_params, jpeg_rows, noise_rows, perspective_coeffs, tone_rows
    from tests.tone_ref import AUTOCONTRAST, COPY, EQUALIZE
    W, H = size
    frame = [(0.0, 0.0), (float(W), 0.0), (float(W), float(H)), (0.0, float(H))]
    quads = [[(1.5 + b, 2.0), (W - 3.0, 0.5 * b), (W - 1.0 - b, H - 2.5), (2.0 * b, H - 1.0)] for b in range(n)]
    return dict(persp=[perspective_coeffs(frame, q) for q in quads], blur=[blur_box_params(r) for r in [0.0, 0.7, 2.0, 5.0][:n]],
                noise=noise_rows([(0, 0, 0.0, 0.0), (7, 9, 2.0, 0.0), (0xDEADBEEF, 1, 0.0, 0.5), (3, 0xFFFFFFFF, 4.0, 1.0)][:n]),
                jpeg=jpeg_rows([0, 50, 90, 10][:n]), tone=tone_rows([(COPY, 0.0), (EQUALIZE, 0.0), (AUTOCONTRAST, 5.0), (AUTOCONTRAST, 0.0)][:n], W * H))


def _stages(front, behind, late, tables):
    """The keyword arguments of one combination.  persp takes the warp slot: with an affine stage the matrix is folded into the homography
    (the two tables together are refused)."""
    from structuredetector_amd.data import compose_affine_perspective
    kw = dict(front); kw.update(behind); kw.update({name: tables[name] for name in late})
    if "persp" in late and "affine" in kw:
        kw["persp"] = [compose_affine_perspective(m, p) for m, p in zip(kw.pop("affine"), tables["persp"])]
    return kw


def _check(x, table, src, out_size, geom, kw, tag):
    """Packed and list chain == the lowest legacy form that takes every stage of kw, packed and list; packed == list."""
    from structuredetector_amd.data import preprocess_image_list, preprocess_images
    from structuredetector_amd.data.augment import _MEAN, _STD
    from tests.helpers import call_legacy_preprocess_form
    form = next((name for name in LEGACY_ORDER if name in kw or name in geom), "")
    arg = lambda name: kw.get(name, geom.get(name))
    args = (x.shape[0], src[0], src[1], out_size, arg("flips"), _MEAN, _STD, arg("jitter"), arg("affine"), arg("mosaic"), arg("window"), arg("letterbox"),
            arg("blur"), x.device, arg("persp"), arg("jpeg"), arg("tone"), arg("noise"))
    packed = preprocess_images(x, out_size, **geom, **kw)
    listed = preprocess_image_list(table, src[0], src[1], out_size, **geom, **kw)
    name = "sd_preprocess_images" + ("_" + form if form else "")
    assert torch.equal(packed, call_legacy_preprocess_form(name, x.data_ptr(), *args)), f"packed {tag} vs {name}"
    name = "sd_preprocess_images_list" + ("_" + form if form else "")
    assert torch.equal(listed, call_legacy_preprocess_form(name, table.data_ptr(), *args)), f"list {tag} vs {name}"
    assert torch.equal(packed, listed), f"packed vs list {tag}"
    return packed


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_chain_equals_the_lowest_legacy_form_bit_for_bit(geometry):
    x = torch.tensor(_sources(), device=DEV)
    arena, table = _table()
    geom = _geometry(geometry)
    tables = _late_tables(OUT, x.shape[0])
    seen = {}
    for name, front, behind in _stage_sets():
        for late in LATE_SETS:
            seen[(name, late)] = _check(x, table, SRC, OUT, geom, _stages(front, behind, late, tables), f"{geometry} {name} {late}")
    for name, _, _ in _stage_sets():                                 # every late stage changes the tensor: none was dropped on the way
        for late in LATE_SETS[1:6]:
            assert not torch.equal(seen[(name, late)], seen[(name, ())]), f"{geometry} {name} {late}"
    del arena


@pytest.mark.parametrize("geometry", ["stretch", "window", "letterbox"])
def test_chain_on_a_batch_of_one_the_smallest_jpeg_frame_and_an_odd_frame(geometry):
    from structuredetector_amd.data import letterbox_geometry
    from tests.test_gpu_image_cache import _arena_with
    from tests.test_gpu_train_tiles import FLIPS, _jitter, _mosaic, _warps
    every = ("persp", "blur", "noise", "jpeg", "tone")
    for n, out_size, late in ((1, OUT, every), (4, (16, 16), every), (4, (31, 27), every[:3] + every[4:])):
        imgs = _sources()[:n]
        x = torch.tensor(imgs, device=DEV)
        arena, addrs = _arena_with(list(imgs), np.random.default_rng(5))
        table = torch.tensor(addrs, dtype=torch.int64, device=DEV)
        geom = {"stretch": {}, "window": dict(window=((48, 40), [(0, 0), (16, 8), (7, 3), (11, 5)][:n])),
                "letterbox": dict(letterbox=letterbox_geometry((SRC[1], SRC[0]), out_size))}[geometry]
        tables = _late_tables(out_size, n)
        front, behind = dict(affine=_warps(out_size, n), mosaic=_mosaic(out_size, n)), dict(flips=FLIPS[:n], jitter=_jitter(n))
        for stages in ((front, behind), ({}, {})):
            got = _check(x, table, SRC, out_size, geom, _stages(*stages, late, tables), f"{geometry} B={n} {out_size} {sorted(stages[0])}")
            assert got.shape == (n, 3, out_size[1], out_size[0]) and torch.isfinite(got).all()
        del arena
