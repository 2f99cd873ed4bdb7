"""Device-resident cache of decoded images for directory-fed training (`--cache_images GB`).

Every epoch of `train --train_dir` decodes every PNG / JPEG again on the host and copies the bytes over PCIe; the GPU work after that
(resize, jitter, flips, normalise, targets) is quick.  Multi-scale training draws a new input size per epoch and Pillow's resample starts
from the original pixels, so what can be kept between epochs is the DECODED ORIGINAL: this cache keeps it in HBM, as uint8 (H, W, 3)
images bump-allocated in a few large arena tensors, up to a byte budget.  A cached sample then costs no decode, no pinned staging and no
PCIe copy: its batch reaches the GPU pipeline as a table of device addresses (`ImageList`), which `preprocess_image_list`
(sd_preprocess_images_list*: a horizontal pass that stages source rows in LDS with 16-byte loads) reads in place.

  * Entries are keyed by (resolved image path, st_mtime_ns, st_size), taken BEFORE the decode (a file rewritten meanwhile misses next
    time instead of hitting stale bytes); the parsed ImageAnnotation is cached under its JSON file's key and handed out as a clone --
    the augmentation resizes, flips and clips annotations in place.
  * No eviction: once the budget is spent, further images take the host path (decode + staging + upload) every epoch.
  * Each rank fills the whole set for itself (`prefill`): its shard permutation changes every epoch (trainer.shard_indices), so filling
    only on misses would leave a rank with 1 - (1 - 1/W)^e of the set after e epochs.
"""
from __future__ import annotations

import os
import threading
import time
from pathlib import Path

import torch

GB = 1e9


def file_key(path):
    """(resolved path, st_mtime_ns, st_size) of a file: a rewrite (new size or mtime) gives a new key."""
    p = Path(path).resolve()
    st = os.stat(p)
    return str(p), st.st_mtime_ns, st.st_size


class ImageList:
    """One size group of a batch as device addresses: `pointers` = (n,) int64 device tensor of (h, w, 3) uint8 images (cache entries or
    this batch's uploads); `keep` = the device tensors allocated for this batch that the addresses point into, besides the cache's arenas."""

    def __init__(self, pointers, height, width, keep=()):
        self.pointers, self.height, self.width, self.keep = pointers, int(height), int(width), list(keep)

    def __len__(self):
        return self.pointers.numel()

    def record_stream(self, stream):
        for t in [self.pointers] + self.keep:
            t.record_stream(stream)


class DeviceImageCache:
    def __init__(self, budget_bytes, device, arena_bytes=1 << 30):
        """budget_bytes: device memory the arenas may take in all; arena_bytes: size of one arena (allocated when the previous one is full)."""
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.budget, self.arena_bytes = int(budget_bytes), int(arena_bytes)
        self._arenas, self._top, self._allocated, self._used = [], 0, 0, 0
        self._images = {}                 # image file key -> (address, height, width)
        self._anns = {}                   # JSON file key -> (ImageAnnotation with img_size, image file)
        self._refused = set()             # image file keys that did not fit
        self._lock = threading.Lock()
        self.hits = self.misses = 0
        self.prefill_seconds = 0.0
        self.fence = None                 # event after the last write into an arena

    def __len__(self):
        return len(self._images)

    def stats(self):
        return {"images": len(self._images), "hits": self.hits, "misses": self.misses, "bytes_used": self._used,
                "bytes_allocated": self._allocated, "refused": len(self._refused), "prefill_seconds": round(self.prefill_seconds, 3)}

    # ---- keys ----
    def keys(self, dataset, index):
        """(JSON key, image key) of sample `index` of a CropDataset; its image file from the cached annotation when there is one (two
        stat calls), else from a parse of its JSON."""
        akey = dataset.annotation_key(index)
        rec = self._anns.get(akey)
        path = rec[1] if rec is not None else dataset.read_annotation(index)[1]
        return akey, file_key(path)

    def lookup(self, dataset, index):
        """((address, height, width), annotation clone) of a cached sample, or None (a miss: counted) when it must be decoded."""
        try:
            akey = dataset.annotation_key(index)
            rec = self._anns.get(akey)
            if rec is not None:
                entry = self._images.get(file_key(rec[1]))
                if entry is not None:
                    with self._lock:
                        self.hits += 1
                    return entry, rec[0].clone()
        except OSError:                   # (a file gone: the host path reports it)
            pass
        with self._lock:
            self.misses += 1
        return None

    def contains(self, dataset, index):
        """Whether sample `index` is cached or known not to fit."""
        try:
            _, ikey = self.keys(dataset, index)
        except OSError:
            return False
        return ikey in self._images or ikey in self._refused

    # ---- insertion: on the CURRENT stream; the caller records `fence` after its batch of inserts ----
    def _alloc(self, nbytes):
        need = (nbytes + 255) // 256 * 256
        if self._arenas and self._top + need <= self._arenas[-1].numel():
            off, self._top = self._top, self._top + need
            return self._arenas[-1], off
        size = max(need, min(self.arena_bytes, self.budget - self._allocated))
        if self._allocated + size > self.budget:
            return None
        arena = torch.empty(size, dtype=torch.uint8, device=self.device)
        self._arenas.append(arena)
        self._allocated += size
        self._top = need
        return arena, 0

    def insert(self, keys, ann, image):
        """Cache one decoded sample: keys from `keys()` (taken before the decode), ann its annotation (a clone is kept), image its
        (h, w, 3) uint8 tensor on this device or in pinned host memory (copied asynchronously on the current stream).  Returns whether
        the image is cached."""
        akey, ikey = keys
        h, w = int(image.shape[0]), int(image.shape[1])
        with self._lock:
            self._anns[akey] = (ann.clone(), Path(ikey[0]))
            if ikey in self._images:
                return True
            if ikey in self._refused:
                return False
            nbytes = h * w * 3
            slot = self._alloc(nbytes)
            if slot is None:
                self._refused.add(ikey)
                return False
            arena, off = slot
            arena[off:off + nbytes].copy_(image.reshape(-1), non_blocking=True)
            self._images[ikey] = (arena.data_ptr() + off, h, w)
            self._used += nbytes
            return True

    def mark_written(self, stream=None):
        """Record `fence` on the stream that ran the inserts: readers wait for it before using new entries."""
        ev = torch.cuda.Event()
        ev.record(stream or torch.cuda.current_stream(self.device))
        self.fence = ev

    def prefill(self, dataset, workers=None, indices=None):
        """Decode every sample of a CropDataset(raw=True) not cached yet on a pool of threads (data/feeder.py: prefetch_items), upload each
        from pinned memory on a side stream into the arenas, and fence with an event (waited for here).  indices: the samples to consider
        (default: all).  Returns the number decoded."""
        from .feeder import prefetch_items
        t0 = time.perf_counter()
        todo = []
        for j in (range(len(dataset)) if indices is None else indices):
            if not self.contains(dataset, j):
                todo.append(j)
        torch.cuda.set_device(self.device)
        side = torch.cuda.Stream(self.device)
        with torch.cuda.stream(side):
            for keys, (img, ann) in prefetch_items(_KeyedReads(self, dataset, todo), workers):
                self.insert(keys, ann, img.pin_memory())
            self.mark_written(side)
        self.fence.synchronize()
        self.prefill_seconds += time.perf_counter() - t0
        return len(todo)


class _KeyedReads:
    """`dataset[indices[k]]` with the cache keys taken before the decode, for prefetch_items."""

    def __init__(self, cache, dataset, indices):
        self.cache, self.dataset, self.indices = cache, dataset, indices

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, k):
        keys = self.cache.keys(self.dataset, self.indices[k])
        return keys, self.dataset[self.indices[k]]


def from_args(args):
    """The cache `--cache_images GB` asks for (None when 0: the feed stays on its host path)."""
    gb = float(getattr(args, "cache_images", 0) or 0)
    if gb < 0:
        raise ValueError(f"--cache_images must be >= 0 (GB of device memory), got {gb}")
    if gb == 0:
        return None
    return DeviceImageCache(int(gb * GB), args.device)
