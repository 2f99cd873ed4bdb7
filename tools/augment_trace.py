#!/usr/bin/env python3
"""Call trace and result digest of the training-augmentation policy layer (`ValidationAugmentation` / `TrainAugmentation` of
structuredetector_amd/data/augment.py and the flag checks of utils/args.py) over a fixed set of configurations.

  record [--out tests/golden/augment_call_trace.json]   write the fixture, on the CPU: per configuration every call the policy makes into
                                                        the three device entry points (recording stand-ins; host tables in full), the
                                                        annotations afterwards and a sha256 of torch's generator state; the descriptors
                                                        `_chain_desc` builds; what the flag checks answer.  The fixture keeps each entry
                                                        as `brief` makes it: names and sizes in the clear, tables behind a digest of their
                                                        full text.  Run it on a checkout of the commit the code under test must equal
                                                        (--root), never on that code.
  diff [--dump DIR]                                     recompute and list every entry that differs from the fixture; --dump (any mode)
                                                        writes the full traces, to compare two checkouts table by table
  digest [--out FILE]                                   on the GPU: the configurations for real, packed and pointer-list forms: sha256 of the
                                                        output tensor and of the annotations: equal bits between two checkouts

--root DIR: the checkout whose `structuredetector_amd` is traced (default: this one)."""
import argparse
import hashlib
import inspect
import json
import math
import sys
from argparse import Namespace
from pathlib import Path
from unittest import mock

HERE = Path(__file__).resolve().parent.parent
FIXTURE = HERE / "tests" / "golden" / "augment_call_trace.json"

SIZE = (64, 64)                                                      # network input (width, height)
SIZES = ((48, 80), (100, 60))                                        # (height, width) of the two source sizes
ORDER = (0, 1, 0, 0, 1, 0, 1, 0)                                     # sample -> source size: 5 + 3, interleaved so that the scatter matters
ALL = dict(aug_rotate=15.0, aug_scale=0.2, aug_translate=0.1, aug_mosaic=0.5, aug_transpose=0.5, aug_blur=2.0, aug_perspective=0.3, aug_jpeg=30,
           aug_equalize=0.3, aug_autocontrast=0.6, aug_autocontrast_cutoff=5.0, aug_noise=6.0, aug_noise_shot=0.5)
TILES = dict(train_tiles="2x2", tile_overlap=32)
STAGES = dict(affine=dict(aug_rotate=15.0, aug_scale=0.2, aug_translate=0.1), mosaic=dict(aug_mosaic=0.5), window=TILES,
              letterbox=dict(keep_aspect=True), transpose=dict(aug_transpose=0.5), blur=dict(aug_blur=2.0), perspective=dict(aug_perspective=0.3),
              jpeg=dict(aug_jpeg=30), tone=dict(aug_equalize=0.3, aug_autocontrast=0.6, aug_autocontrast_cutoff=5.0),
              noise=dict(aug_noise=6.0, aug_noise_shot=0.5))

# name: (train?, flags, options).  Options: form = "list" (arrays; the default) | "tensor" (one 4-D tensor of the first size) | "pointers"
# (an object with .groups whose stacks have .pointers); size = the multi-scale size set before the call; images_at = a second size asked
# from the same images after the call.  The seed of a configuration is its position in this table.
CONFIGS = {
    "validation": (False, {}, {}),
    "validation_keep_aspect": (False, dict(keep_aspect=True), {}),
    "train_defaults": (True, {}, {}),
    "no_augmentation": (True, dict(no_augmentation=True), {}),
    "no_augmentation_train_tiles": (True, dict(no_augmentation=True, **TILES), {}),
    **{f"only_{stage}": (True, flags, {}) for stage, flags in STAGES.items()},
    "affine_perspective": (True, {**STAGES["affine"], **STAGES["perspective"]}, {}),
    "mosaic_always": (True, dict(aug_mosaic=1.0), {}),
    "everything": (True, ALL, {}),
    "everything_train_tiles": (True, {**ALL, **TILES}, {}),
    "everything_keep_aspect": (True, dict(ALL, keep_aspect=True), {}),
    "non_square": (True, {k: v for k, v in ALL.items() if k != "aug_transpose"}, dict(size=(96, 64))),
    "form_list": (True, STAGES["affine"], dict(form="list")),
    "form_tensor": (True, STAGES["affine"], dict(form="tensor")),
    "form_pointers": (True, ALL, dict(form="pointers")),
    "images_at": (False, {}, dict(images_at=(96, 32))),
    "images_at_keep_aspect_pointers": (False, dict(keep_aspect=True), dict(images_at=(96, 32), form="pointers")),
    "refuse_transpose_non_square": (True, dict(aug_transpose=0.5), dict(size=(96, 64))),
    "refuse_window_keep_aspect": (True, dict(keep_aspect=True, **TILES), {}),
}

# (name, geometry arguments, optional tables) of the descriptor cases; the tables are made by `_desc_tables`
DESC_CASES = ([(f"stretch_{t}", {}, (t,)) for t in ("flips", "jitter", "affine", "mosaic", "blur", "persp", "jpeg", "tone", "noise")] +
              [("stretch_plain", {}, ()), ("window_plain", dict(window=True), ()), ("letterbox_plain", dict(letterbox=True), ())] +
              [(f"{g}_all", {g: True} if g != "stretch" else {}, ("flips", "jitter", "mosaic", "blur", "persp", "jpeg", "tone", "noise"))
               for g in ("stretch", "window", "letterbox")] +
              [("list_all_affine", dict(is_list=True), ("flips", "jitter", "affine", "mosaic", "blur", "jpeg", "tone", "noise"))])

# flag: the values the checks are asked about, both ends, just outside them, NaN and True among them (tests/test_augment_trace_cpu.py
# derives the same values from the table of utils/args.py and looks every one of them up here)
NAN = float("nan")
FLAG_PROBES = {
    "aug_rotate": (0.0, 180.0, -0.001, 180.001, NAN, True, 90.0), "aug_scale": (0.0, 1.0, -0.001, 0.999, NAN, True, 0.5),
    "aug_translate": (0.0, 0.5, -0.001, 0.501, NAN, True, 0.25), "aug_mosaic": (0.0, 1.0, -0.001, 1.001, NAN, True, 0.5),
    "aug_transpose": (0.0, 1.0, -0.001, 1.001, NAN, True, 0.5), "aug_blur": (0.0, 8.0, -0.001, 8.001, NAN, True, 4.0),
    "aug_perspective": (0.0, 0.9, -0.001, 0.901, NAN, True, 0.45), "aug_jpeg": (0, 5, 95, 4, 96, -1, NAN, True, 50, 50.0),
    "aug_equalize": (0.0, 1.0, -0.001, 1.001, NAN, True, 0.5), "aug_autocontrast": (0.0, 1.0, -0.001, 1.001, NAN, True, 0.5),
    "aug_autocontrast_cutoff": (0.0, 40.0, -0.001, 40.001, NAN, True, 20.0, None), "aug_noise": (0.0, 32.0, -0.001, 32.001, NAN, True, 16.0),
    "aug_noise_shot": (0.0, 2.0, -0.001, 2.001, NAN, True, 1.0),
}
FLAG_CHECKS = {"aug_transpose": "check_aug_transpose", "aug_blur": "check_aug_blur", "aug_perspective": "check_aug_perspective",
               "aug_jpeg": "check_aug_jpeg", "aug_equalize": "check_aug_tone", "aug_autocontrast": "check_aug_tone",
               "aug_autocontrast_cutoff": "check_aug_tone", "aug_noise": "check_aug_noise", "aug_noise_shot": "check_aug_noise"}
TRAIN_CHECKS = ("check_train_tiles", "check_keep_aspect", "check_aug_transpose", "check_aug_blur", "check_aug_perspective", "check_aug_jpeg",
                "check_aug_tone", "check_aug_noise")                 # what `Trainer.__init__` ran one under the other before `check_train`


def sha(data):
    return hashlib.sha256(data).hexdigest()


def canon(v):
    """A value as JSON keeps it: tensors and arrays become lists (floats round-trip through json exactly), tuples lists."""
    import numpy as np
    import torch
    if isinstance(v, torch.Tensor):
        return {"tensor": list(v.shape), "dtype": str(v.dtype), "values": v.tolist() if v.numel() <= 64 else sha(v.contiguous().numpy().tobytes())}
    if isinstance(v, np.ndarray):
        return canon(v.tolist())
    if isinstance(v, (list, tuple)) or inspect.isgenerator(v):
        return [canon(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return repr(v)
    return v.item() if isinstance(v, np.generic) else v


def make_args(train, flags, device):
    return Namespace(**{**dict(width=SIZE[0], height=SIZE[1], no_augmentation=False, device=device), **flags})


def plain_solve(a, b):
    """`numpy.linalg.solve` for the trace: Gaussian elimination with partial pivoting in Python floats.  LAPACK's answer differs in the last
    bit between CPU families (the BLAS picks its kernels by the CPU), and the fixture must not depend on where it was recorded; the policy
    layer under test only passes the solver's answer on (`perspective_coeffs`)."""
    import numpy as np
    n = len(b)
    m = [[float(v) for v in row] + [float(b[i])] for i, row in enumerate(a)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(m[r][c]))
        m[c], m[p] = m[p], m[c]
        for r in range(c + 1, n):
            f = m[r][c] / m[c][c]
            for k in range(c, n + 1):
                m[r][k] -= f * m[c][k]
    x = [0.0] * n
    for r in reversed(range(n)):
        x[r] = (m[r][n] - sum(m[r][k] * x[k] for k in range(r + 1, n))) / m[r][r]
    return np.asarray(x)


def make_images(form, device):
    """(what `__call__` takes as images, n): seeded bytes, the 5 + 3 samples of the two source sizes in the order ORDER."""
    import numpy as np
    import torch
    rng = np.random.default_rng(5)
    order = (0,) * len(ORDER) if form == "tensor" else ORDER
    arrays = [rng.integers(0, 256, (*SIZES[k], 3), dtype=np.uint8) for k in order]
    if form == "list":
        return arrays
    if form == "tensor":
        return torch.from_numpy(np.stack(arrays)).to(device)
    groups, keep = {}, []
    for hw in SIZES:                                                 # "packed" (stacks) and "pointers" (addresses): what data/feeder.py makes
        idx = [i for i, k in enumerate(order) if SIZES[k] == hw]
        stack = torch.from_numpy(np.stack([arrays[i] for i in idx])).to(device)
        if form == "pointers":
            keep.append(stack)
            addresses = [stack[k].data_ptr() for k in range(len(idx))] if stack.is_cuda else [1000 * hw[0] + k for k in range(len(idx))]
            stack = Namespace(pointers=torch.tensor(addresses, dtype=torch.int64, device=device), height=hw[0], width=hw[1])
        groups[hw] = (idx, stack)
    return Namespace(groups=groups, keep=keep)


def make_annotations():
    """Four objects with one part each per sample, in source pixels: two hug the borders (a warp or a window drops them), two sit inside."""
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    anns = []
    for i, k in enumerate(ORDER):
        h, w = SIZES[k]
        spots = ((0.03, 0.05), (0.5 + 0.01 * i, 0.5), (0.97, 0.9 - 0.01 * i), (0.3, 0.72))
        anns.append(ImageAnnotation(f"/trace/img{i}.png", [Object(f"l{j % 2}", Keypoint("anchor", fx * w, fy * h), [Keypoint("p0", min(fx + 0.04, 0.995) * w, fy * h)])
                                                             for j, (fx, fy) in enumerate(spots)]))
    return anns


def build(name, device):
    import torch

    from structuredetector_amd.data import augment as A
    train, flags, opts = CONFIGS[name]
    aug = (A.TrainAugmentation if train else A.ValidationAugmentation)(make_args(train, flags, device))
    if "size" in opts:
        aug.size = opts["size"]
    torch.manual_seed(100 + list(CONFIGS).index(name))
    return aug, opts


class Recorder:
    """Stand-ins of `preprocess_images`, `preprocess_image_list` and `transpose_select`: every call with its arguments by name."""

    def __init__(self, module):
        self.module, self.calls = module, []
        self.real = {n: getattr(module, n) for n in ("preprocess_images", "preprocess_image_list", "transpose_select")}

    def stand_in(self, fn_name):
        import torch

        def call(*a, **k):
            bound = inspect.signature(self.real[fn_name]).bind(*a, **k)
            bound.apply_defaults()
            given = dict(bound.arguments)
            first = given.pop(next(iter(given)))                     # images / pointers / batch
            if fn_name == "transpose_select":
                self.calls.append({"fn": fn_name, "batch": list(first.shape), "select": canon(given["select"])})
                return first.clone()
            entry = {"fn": fn_name, "B": first.shape[0], "source": canon(first)}
            entry.update({key: canon(value) for key, value in given.items()})
            self.calls.append(entry)
            w, h = given["out_size"]
            return torch.full((first.shape[0], 3, h, w), float(len(self.calls)))
        return call

    def __enter__(self):
        for n in self.real:
            setattr(self.module, n, self.stand_in(n))
        return self

    def __exit__(self, *exc):
        for n, fn in self.real.items():
            setattr(self.module, n, fn)


def trace_config(name):
    """One configuration on the CPU -> {calls, annotations, rng, out (where each sample's rows came from) | error}."""
    import torch

    from structuredetector_amd.data import augment as A
    dev = torch.device("cpu")
    aug, opts = build(name, dev)
    images, anns = make_images(opts.get("form", "list"), dev), make_annotations()
    result = {}
    with Recorder(A) as rec, mock.patch("numpy.linalg.solve", plain_solve):
        try:
            out, anns = aug(images, anns)
            result["out"] = {"shape": list(out.shape), "call_of_sample": out[:, 0, 0, 0].tolist()}
            if "images_at" in opts:
                other = aug.images_at(images, opts["images_at"])
                result["images_at"] = {"shape": list(other.shape), "call_of_sample": other[:, 0, 0, 0].tolist()}
        except Exception as e:                                      # the two refusals
            result["error"] = [type(e).__name__, str(e)]
    result.update(calls=rec.calls, annotations=[a.json_repr() for a in anns], rng=sha(torch.get_rng_state().numpy().tobytes()))
    return result


def _desc_tables(n, size):
    """The optional tables of a descriptor case, by the argument name of `_chain_desc`, made with the project's arithmetic helpers."""
    from structuredetector_amd.data import augment as A
    W, H = size
    inv = [A.affine_inverse_matrix(size, 7.0 * i - 10, 1.0 + 0.05 * i, (1.5 * i, -2.0 * i)) for i in range(n)]
    frame = [(0.0, 0.0), (float(W), 0.0), (float(W), float(H)), (0.0, float(H))]
    quad = [(2.0, 1.0), (W - 3.0, 2.5), (W - 1.0, H - 4.0), (1.5, H - 2.0)]
    tiles = [A.mosaic_tiles(size, i, (W // 2 + i, H // 2 - i, ((i + 1) % n, (i + 2) % n, i)) if i % 2 else None) for i in range(n)]
    jit = [A.jitter_words((i % 4, (i + 1) % 4, (i + 2) % 4, (i + 3) % 4), 1.1, 0.9, 1.05, 0.01 * i) for i in range(n)]
    return dict(flips=[i % 4 for i in range(n)], jitter=([w for w, _ in jit], [f for _, f in jit]), affine=inv,
                persp=[A.compose_affine_perspective(inv[i], A.perspective_coeffs(frame, quad)) for i in range(n)],
                mosaic=([t[0] for t in tiles], [t[1] for t in tiles]), blur=[A.blur_box_params(0.5 * i) for i in range(n)],
                jpeg=A.jpeg_rows([0, 30, 75, 95][i % 4] for i in range(n)), tone=A.tone_rows([(i % 3, 2.5 * i) for i in range(n)], W * H),
                noise=A.noise_rows([(2 ** 31 + i, 12345 * i, 1.5 * i, 0.25 * i) for i in range(n)]))


def trace_descriptors():
    """`_chain_desc` on CPU tensors (it makes no library call) -> per case the scalar fields, which pointer fields are set and a sha256
    of every kept table's bytes, by the field that points at it."""
    import ctypes as C

    import torch

    from structuredetector_amd.data import augment as A
    dev, n, (hin, win), size = torch.device("cpu"), 4, SIZES[0], (64, 32)
    source = torch.zeros(n, hin, win, 3, dtype=torch.uint8)
    with mock.patch("numpy.linalg.solve", plain_solve):
        tables, out = _desc_tables(n, size), {}
    for name, geometry, wanted in DESC_CASES:
        opt = {k: (tables[k] if k in wanted else None) for k in ("flips", "jitter", "affine", "mosaic", "blur", "persp", "jpeg", "tone", "noise")}
        window = ((100, 50), [(3 * i, 2 * i) for i in range(n)]) if geometry.get("window") else None
        letterbox = (53, 32, 5, 0) if geometry.get("letterbox") else None
        d, res, keep = A._chain_desc(source.data_ptr(), bool(geometry.get("is_list")), n, hin, win, size, opt["flips"], A._MEAN, A._STD, opt["jitter"],
                                     opt["affine"], opt["mosaic"], window, letterbox, opt["blur"], opt["persp"], opt["jpeg"], opt["tone"],
                                     opt["noise"], dev)
        by_address = {t.data_ptr(): t for t in keep if t is not None}
        entry = {"out": [list(res.shape), str(res.dtype)], "scalars": {}, "tables": {}}
        for field, kind in A.L.PreprocessDesc._fields_:
            v = getattr(d, field)
            if field in ("fill3", "mean3", "std3"):
                entry["scalars"][field] = [v[i] for i in range(3)]
            elif kind is C.c_int:
                entry["scalars"][field] = v
            elif field not in ("images", "out"):
                t = by_address.get(v) if v else None
                entry["tables"][field] = None if not v else [list(t.shape), str(t.dtype), sha(t.contiguous().numpy().tobytes())]
        out[name] = entry
    return out


def outcome(fn, *a, **k):
    try:
        return ["ok", repr(fn(*a, **k))]
    except Exception as e:
        return [type(e).__name__, str(e)]


def probe_key(flag, value, synthetic):
    return f"{flag}={value!r}" + (" --synthetic" if synthetic else "")


def trace_flag(flag, value, synthetic):
    """What the checks answer for one value of one flag: {"check": its `check_aug_*` (if it has one), "train": everything `train` checks,
    "finalize": the parser's validation (as a machine without a GPU ends it: the RuntimeError after the last assert = accepted),
    "policy": the attributes `TrainAugmentation.__init__` reads}."""
    from structuredetector_amd.data import augment as A
    from structuredetector_amd.utils import args as M
    parser = M.Arguments().parser
    ns = parser.parse_args(["--synthetic", "8"] if synthetic else [])
    setattr(ns, flag, value)
    ns.labels, ns.parts = {"l0": 0}, {"p0": 0}
    res = {}
    if flag in FLAG_CHECKS:
        res["check"] = outcome(getattr(M, FLAG_CHECKS[flag]), ns)
    if hasattr(M, "check_train"):
        res["train"] = outcome(lambda: M.check_train(ns) and None)
    else:
        res["train"] = outcome(lambda: [getattr(M, c)(ns, training=True) if c == "check_keep_aspect" else getattr(M, c)(ns) for c in TRAIN_CHECKS] and None)
    with mock.patch("torch.cuda.is_available", return_value=False):
        res["finalize"] = outcome(M.finalize, Namespace(**vars(ns)))
    policy = outcome(lambda: sorted((k, v) for k, v in vars(A.TrainAugmentation(Namespace(**vars(ns), device=None))).items()
                                    if isinstance(v, (int, float, tuple)) and k != "prob"))
    res["policy"] = policy
    return res


def trace_absent():
    """A Namespace from before every flag: what the checks, the policy's attributes and the parser give."""
    from structuredetector_amd.data import augment as A
    from structuredetector_amd.utils import args as M
    old = Namespace(width=64, height=64, no_augmentation=False, device=None)
    return {"checks": {c: outcome(getattr(M, c), old) for c in sorted(set(FLAG_CHECKS.values()))},
            "policy": outcome(lambda: sorted((k, v) for k, v in vars(A.TrainAugmentation(old)).items()
                                             if isinstance(v, (int, float, tuple)) and k != "prob")),
            "parser": {flag: repr(getattr(M.Arguments().parser.parse_args([]), flag)) for flag in FLAG_PROBES}}


def trace_flags():
    out = {probe_key(flag, v, s): trace_flag(flag, v, s) for flag, values in FLAG_PROBES.items() for v in values for s in (0, 8)}
    out["absent"] = trace_absent()
    return out


def trace_all():
    return {"configs": {name: trace_config(name) for name in CONFIGS}, "descriptors": trace_descriptors(), "flags": trace_flags()}


def digest_config(name, form):
    """One configuration for real on the GPU -> {out, annotations (+ images_at)}: sha256 each, or the refusal."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    aug, opts = build(name, dev)
    images, anns = make_images("tensor" if opts.get("form") == "tensor" else form, dev), make_annotations()
    try:
        out, anns = aug(images, anns)
        res = {"out": sha(out.cpu().contiguous().numpy().tobytes())}
        if "images_at" in opts:
            res["images_at"] = sha(aug.images_at(images, opts["images_at"]).cpu().contiguous().numpy().tobytes())
    except Exception as e:
        res = {"error": [type(e).__name__, str(e)]}
    torch.cuda.synchronize()
    res["annotations"] = sha(json.dumps([a.json_repr() for a in anns]).encode())
    res["rng"] = sha(torch.get_rng_state().numpy().tobytes())
    return res


def tag(v):
    """48 bits of the sha256 of a value's JSON text (floats in full): what the fixture keeps in the place of a table."""
    return sha(json.dumps(v, sort_keys=True).encode())[:12]


def brief(part, entry):
    """What the fixture keeps of one traced entry of `part` (configs / descriptors / flags): what names a difference -- the call, its
    sizes, which tables it got, the object counts, the outcome types -- in the clear, and every table, annotation and message behind a
    `tag` of its full text.  `diff --dump DIR` writes the full traces of a checkout, to be compared file by file."""
    entry = json.loads(json.dumps(entry))
    if part == "configs":
        calls = []
        for c in entry["calls"]:
            if c["fn"] == "transpose_select":
                calls.append(f"transpose_select batch={c['batch']} #{tag(c)}")
            else:
                given = ",".join(k for k, v in c.items() if v is not None and k not in ("fn", "B", "source", "out_size", "mean", "std", "hin", "win"))
                calls.append(f"{c['fn']} B={c['B']} out={c['out_size']} {given} #{tag(c)}")
        out = {"calls": calls, "objects": ",".join(str(len(a["objects"])) for a in entry["annotations"]), "annotations": tag(entry["annotations"]),
               "rng": entry["rng"][:12], "out": tag([entry.get("out"), entry.get("images_at")])}
        return {**out, "error": entry["error"]} if "error" in entry else out
    if part == "descriptors":
        ints = {k: v for k, v in entry["scalars"].items() if isinstance(v, int)}
        return {"scalars": " ".join(f"{k}={v}" for k, v in ints.items()) + f" #{tag(entry['scalars'])}",
                "tables": ",".join(k for k, v in entry["tables"].items() if v is not None) + f" #{tag([entry['tables'], entry['out']])}"}
    if "parser" in entry:                                            # flags: the namespace from before every flag
        return {"parser": entry["parser"], "checks_and_policy": tag([entry["checks"], entry["policy"]])}
    return " ".join(f"{k}={v[0]}" for k, v in entry.items()) + f" #{tag(entry)}"


def brief_all(trace):
    return {part: {name: brief(part, entry) for name, entry in entries.items()} for part, entries in trace.items()}


def differences(got, want, path=""):
    """The paths at which two recorded structures differ (NaN never occurs in them: non-finite floats are kept as text)."""
    if isinstance(got, dict) and isinstance(want, dict):
        return [d for k in sorted(set(got) | set(want)) for d in
                ([f"{path}/{k}: only {'here' if k in got else 'recorded'}"] if (k in got) != (k in want) else differences(got[k], want[k], f"{path}/{k}"))]
    if isinstance(got, list) and isinstance(want, list) and len(got) == len(want):
        return [d for i, (g, w) in enumerate(zip(got, want)) for d in differences(g, w, f"{path}[{i}]")]
    return [] if got == want and type(got) is type(want) else [f"{path}: {str(got)[:120]} here, {str(want)[:120]} recorded"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("record", "diff", "digest"))
    ap.add_argument("--root", default=str(HERE)); ap.add_argument("--out", default=None); ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.root).resolve()))
    if a.mode == "digest":
        import structuredetector_amd
        print(f"digest of {structuredetector_amd.__file__}", file=sys.stderr)
        table = {f"{name}/{form}": digest_config(name, form) for name in CONFIGS for form in ("packed", "pointers")}
        text = json.dumps(table, indent=1)
        print(text)
        if a.out:
            Path(a.out).write_text(text + "\n")
        return 0
    full = json.loads(json.dumps(trace_all()))
    if a.dump:
        Path(a.dump).mkdir(parents=True, exist_ok=True)
        for part, entries in full.items():
            (Path(a.dump) / f"{part}.json").write_text(json.dumps(entries, indent=1, sort_keys=True) + "\n")
    got = brief_all(full)
    if a.mode == "record":
        out = Path(a.out or FIXTURE)
        out.write_text(json.dumps(got, indent=1) + "\n")
        print(f"{out}: {', '.join(f'{len(v)} {k}' for k, v in got.items())}, {out.stat().st_size} bytes")
        return 0
    bad = differences(got, json.loads(FIXTURE.read_text()))
    print("\n".join(bad) if bad else f"equal: {', '.join(f'{len(v)} {k}' for k, v in got.items())}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
