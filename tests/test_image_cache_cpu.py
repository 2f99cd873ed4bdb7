"""Device-resident decoded-image cache (`--cache_images`, data/image_cache.py) and its entry points
(sd_preprocess_images_list[_jitter]): the parts that run without a GPU -- argument validation of the C ABI, the flag, the cache keys."""
import os
from argparse import Namespace

import numpy as np
import pytest

SD_ERR_INVALID, SD_ERR_WORKSPACE = -1, -2


def test_list_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Every check runs before a launch: a null table, B <= 0, B > 65535 on the jitter form, null coefficient tables, rows too wide
    for the LDS staging buffer and a short workspace return an SD_ERR_* code and set sd_last_error()."""
    import ctypes as C
    from structuredetector_amd import _lib as L
    lib = L.lib()
    m3, s3 = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.2, 0.2, 0.2)
    P = 16                                                               # a non-null stand-in: never dereferenced

    def plain(table=P, B=2, Hin=8, Win=8, hb=P, hk=P, vb=P, vk=P, ws=1 << 20):
        return lib.sd_preprocess_images_list(table, B, Hin, Win, 4, 4, hb, hk, 3, vb, vk, 3, 0, m3, s3, P, P, ws, 0)

    def jitter(table=P, B=2, Hin=8, Win=8, hb=P, hk=P, vb=P, vk=P, order=P, factors=P, ws=1 << 20):
        return lib.sd_preprocess_images_list_jitter(table, B, Hin, Win, 4, 4, hb, hk, 3, vb, vk, 3, 0, order, factors, m3, s3, P, P, ws, 0)

    for fn, name in ((plain, b"sd_preprocess_images_list"), (jitter, b"sd_preprocess_images_list_jitter")):
        assert fn(table=0) == SD_ERR_INVALID and name in lib.sd_last_error()
        assert fn(B=0) == SD_ERR_INVALID and b"bad shape" in lib.sd_last_error()
        assert fn(B=-3) == SD_ERR_INVALID
        for k in ("hb", "hk", "vb", "vk"):
            assert fn(**{k: 0}) == SD_ERR_INVALID and b"null pointer" in lib.sd_last_error()
        assert fn(Win=21835) == SD_ERR_INVALID and b"LDS" in lib.sd_last_error()
        assert fn(ws=16) == SD_ERR_WORKSPACE and b"workspace" in lib.sd_last_error()
    assert jitter(B=65536) == SD_ERR_INVALID and b"65535" in lib.sd_last_error()
    assert jitter(order=0) == SD_ERR_INVALID and b"jitter" in lib.sd_last_error()
    assert jitter(factors=0) == SD_ERR_INVALID
    # the widest row the LDS staging takes passes validation up to the workspace check (nothing launched)
    assert plain(Win=21834, ws=16) == SD_ERR_WORKSPACE


def test_cache_images_flag():
    """--cache_images GB: default 0 = no cache (the feed stays on its host path), a negative value is refused."""
    from structuredetector_amd.data import BatchFeeder
    from structuredetector_amd.data.image_cache import DeviceImageCache, from_args
    from structuredetector_amd.utils.args import Arguments
    parser = Arguments().parser
    assert parser.parse_args([]).cache_images == 0
    assert parser.parse_args(["--cache_images", "2.5"]).cache_images == 2.5
    with pytest.raises(AssertionError, match="cache_images"):
        Arguments().parse(["--cache_images", "-1"])
    with pytest.raises(ValueError):
        from_args(Namespace(cache_images=-1.0, device="cuda:0"))
    assert from_args(Namespace(cache_images=0.0, device="cuda:0")) is None
    cache = from_args(Namespace(cache_images=0.25, device="cuda:0"))
    assert isinstance(cache, DeviceImageCache) and cache.budget == 250_000_000 and len(cache) == 0
    # without a cache the feeder takes its old path: whole-tensor size groups (no pointer tables)
    assert BatchFeeder([], [[0]], "cuda:0").cache is None
    assert BatchFeeder([], [[0]], "cuda:0", cache=cache).cache is cache


def test_dataset_split_and_cache_keys(golden_dir, tmp_path):
    """CropDataset's annotation-only read and per-sample keys: the annotation equals __getitem__'s (minus the decoded size), the key of an
    image changes when the file is rewritten (new size or new mtime), and a lookup in an empty cache is a counted miss."""
    from structuredetector_amd.data import CropDataset
    from structuredetector_amd.data.image_cache import DeviceImageCache, file_key
    from tests.helpers import EVAL16_LABELS, EVAL16_PARTS, write_evaluate16_dir
    g = np.load(golden_dir / "evaluate16.npz")
    write_evaluate16_dir(g, tmp_path / "train")
    args = Namespace(labels=EVAL16_LABELS, parts=EVAL16_PARTS, width=128, height=128, anchor_name="stem")
    ds = CropDataset(args, tmp_path / "train", raw=True)
    img, full = ds[3]
    ann, path = ds.read_annotation(3)
    assert path == tmp_path / "train" / "img_03.png" and ann.image_path == full.image_path
    assert [(o.name, o.anchor.x, o.anchor.y) for o in ann.objects] == [(o.name, o.anchor.x, o.anchor.y) for o in full.objects]
    assert tuple(full.img_size) == (img.shape[1], img.shape[0])
    cache = DeviceImageCache(1 << 20, "cuda:0")
    akey, ikey = cache.keys(ds, 3)
    assert akey == ds.annotation_key(3) and ikey == file_key(path) and ikey[0] == str(path.resolve())
    from PIL import Image
    Image.open(path).resize((64, 48)).save(path)                          # new size
    assert cache.keys(ds, 3)[1] != ikey
    k2 = cache.keys(ds, 3)[1]
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))   # same bytes, new mtime
    assert cache.keys(ds, 3)[1] not in (ikey, k2)
    assert cache.lookup(ds, 3) is None and not cache.contains(ds, 3)
    assert cache.stats()["misses"] == 1 and cache.stats()["hits"] == 0 and cache.stats()["images"] == 0
