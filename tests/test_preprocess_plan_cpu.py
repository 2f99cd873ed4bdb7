"""The preprocess chain's plan (csrc/sd_image.hip plan_chain) without a GPU: sd_preprocess_kernel_names for every combination of geometry,
source form and stages against the launch table written out below, the refusals of sd_preprocess_chain (it returns before any launch; the
pointers are never dereferenced), and sd_preprocess_chain_workspace_bytes against the legacy size queries."""
import ctypes as C
import itertools
import re

import pytest

B, HIN, WIN, HOUT, WOUT = 4, 40, 56, 32, 32
CANVAS = (48, 40)                                                    # the window geometry's canvas (width, height)
P = 4096                                                             # a non-null stand-in for a device pointer: never dereferenced
GEOMETRIES = ["stretch", "window", "letterbox"]
H_KERNEL = {"stretch": "k_resample_h", "window": "k_window_h", "letterbox": "k_resample_h"}
V_KERNEL = {"stretch": "k_resample_v", "window": "k_window_v", "letterbox": "k_letterbox_v"}
J = [("k_jitter_lsum", "sums"), ("k_jitter_norm", "out")]
# the launches after H without a late stage, "V" standing for the geometry's vertical kernel: (kernel, dst)
NOT_LATE = {
    (): [("V_norm", "out")],
    ("jitter",): [("V_u8", "A")] + J,
    ("affine",): [("V_u8", "B"), ("k_affine_norm", "out")],
    ("affine", "jitter"): [("V_u8", "B"), ("k_affine_u8", "A")] + J,
    ("mosaic",): [("V_u8", "B"), ("k_mosaic_norm", "out")],
    ("mosaic", "jitter"): [("V_u8", "B"), ("k_mosaic_u8", "A")] + J,
    ("mosaic", "affine"): [("V_u8", "A"), ("k_mosaic_u8", "B"), ("k_affine_norm", "out")],
    ("mosaic", "affine", "jitter"): [("V_u8", "A"), ("k_mosaic_u8", "B"), ("k_affine_u8", "A")] + J,
}
# the late path's 8-bit stages in front of the blur alternate so that the last writes A: the dst of V [, mosaic] [, warp]
LATE_FRONT = {(False, False): ["A"], (True, False): ["B", "A"], (False, True): ["B", "A"], (True, True): ["A", "B", "A"]}
LATE_SETS = [(), ("blur",), ("persp",), ("noise",), ("jpeg",), ("tone",), ("persp", "blur", "noise", "jpeg", "tone")]
CASES = list(itertools.product(GEOMETRIES, (False, True), NOT_LATE, LATE_SETS))


def _align(n):
    return (n + 255) // 256 * 256


def _geometry(name):
    """geometry id, Hg, Wg, g0, g1 as sd_preprocess_desc documents them (a number: that id with the stretch's zeros)."""
    from structuredetector_amd.data import letterbox_geometry
    from structuredetector_amd.data.augment import window_extents
    if isinstance(name, int):
        return name, 0, 0, 0, 0
    if name == "window":
        return 1, CANVAS[1], CANVAS[0], window_extents(HIN, CANVAS[1], HOUT), window_extents(WIN, CANVAS[0], WOUT)
    if name == "letterbox":
        wi, hi, px, py = letterbox_geometry((WIN, HIN), (WOUT, HOUT))
        return 2, hi, wi, py, px
    return 0, 0, 0, 0, 0


def _desc(geometry="stretch", is_list=False, stages=(), late=(), **over):
    """A descriptor with fake non-null pointers; keeps its host arrays alive.  persp takes the warp slot: a row with affine and persp hands
    its warp over as the homography (the two together are refused, see the rejections)."""
    from structuredetector_amd import _lib as L
    d = L.PreprocessDesc(images=P, list=int(is_list), B=B, Hin=HIN, Win=WIN, Hout=HOUT, Wout=WOUT, h_bounds=P, h_kk=P, h_ksize=3, v_bounds=P, v_kk=P,
                         v_ksize=3, out=P)
    d.geometry, d.Hg, d.Wg, d.g0, d.g1 = _geometry(geometry)
    d.window = P if geometry == "window" else None
    d.fill3, d.mean3, d.std3 = (C.c_ubyte * 3)(124, 116, 104), (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25)
    if "jitter" in stages:
        d.jitter_order = d.jitter_factors = P
    if "mosaic" in stages:
        d.mosaic_geom = d.mosaic_affine = P
    if "affine" in stages and "persp" not in late:
        d.affine = P
    for name in late:
        setattr(d, name, P)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _names(d):
    from structuredetector_amd import _lib as L
    return L.lib().sd_preprocess_kernel_names(C.byref(d)).decode()


def _expected(geometry, is_list, stages, late):
    """[(kernel or token, dst or None)] from the table above."""
    v = lambda k: k.replace("V", V_KERNEL[geometry], 1) if k.startswith("V_") else k
    seq = [("memset", None)] if "jitter" in stages else []
    seq.append((H_KERNEL[geometry] + ("_list" if is_list else ""), "tmp"))
    if not late:
        return seq + [(v(k), dst) for k, dst in NOT_LATE[stages]]
    mosaic, warp = "mosaic" in stages, "affine" in stages or "persp" in late
    front = ["V_u8"] + (["k_mosaic_u8"] if mosaic else []) + (["k_persp_u8" if "persp" in late else "k_affine_u8"] if warp else [])
    seq += [(v(k), dst) for k, dst in zip(front, LATE_FRONT[(mosaic, warp)])]
    seq += [(name, None) for name in ("blur", "noise", "jpeg", "tone") if name in late]        # on A, in this order
    return seq + (J if "jitter" in stages else [("k_u8_norm", "out")])


def _parse(line):
    """"<kernel> grid=XxYxZ block=T lds=N dst=D" -> (kernel, dst, grid, block, lds); a bare token -> (token, None, None, None, None)."""
    out = []
    for part in line.split("; "):
        m = re.fullmatch(r"(\S+) grid=(\d+)x(\d+)x(\d+) block=(\d+) lds=(\d+) dst=(\w+)", part)
        out.append((m.group(1), m.group(7), tuple(int(m.group(i)) for i in (2, 3, 4)), int(m.group(5)), int(m.group(6))) if m else
                   (part, None, None, None, None))
    return out


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_kernel_names_follow_the_launch_table(geometry):
    cdiv = lambda a, b: -(-a // b)
    gid, Hg, Wg, g0, g1 = _geometry(geometry)
    rows, cols = (g0 if geometry == "window" else HIN), (Wg if geometry == "letterbox" else WOUT)
    span = g1 if geometry == "window" else WIN
    rpb = min(4, (65536 - 32) // (span * 3))
    flat = (cdiv(B * HOUT * WOUT, 256), 1, 1)
    for geo, is_list, stages, late in CASES:
        if geo != geometry:
            continue
        line = _names(_desc(geometry, is_list, stages, late))
        got = _parse(line)
        what = f"{geometry} list={is_list} {stages} {late}: {line}"
        assert [(k, dst) for k, dst, *_ in got] == _expected(geometry, is_list, stages, late), what
        assert ("memset" in line) == ("jitter" in stages) and line.startswith("memset") == ("jitter" in stages), what
        for kernel, dst, grid, block, lds in got:
            if grid is None:
                continue
            assert block == 256, what
            if kernel.endswith("_h_list"):
                assert lds == rpb * span * 3 + 32 and grid == (B * cdiv(rows, rpb), 1, 1), what
                continue
            assert lds == 0, what
            if kernel.endswith("_h"):
                assert grid == (cdiv(B * rows * cols, 256), 1, 1), what
            elif kernel in ("k_mosaic_u8", "k_mosaic_norm", "k_affine_u8", "k_affine_norm", "k_persp_u8"):
                assert grid == (cdiv(WOUT, 64), cdiv(HOUT, 16), B), what
            elif kernel == "k_jitter_lsum":
                assert grid == (min(cdiv(HOUT * WOUT, 256), 64), B, 1), what
            else:                                                    # the vertical kernels, k_jitter_norm, k_u8_norm
                assert grid == flat, what


def test_chain_rejects_what_the_legacy_forms_reject():
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def run(d, ws=P, nbytes=1 << 30):
        lib.sd_set_option(b"no_such_option", 1)                      # leaves another message behind
        rc = lib.sd_preprocess_chain(C.byref(d) if d is not None else None, ws, nbytes, 0)
        return rc, lib.sd_last_error().decode()

    def refused(text, d, code=-1, **kw):
        rc, msg = run(d, **kw)
        assert rc == code and "sd_preprocess_chain" in msg and re.search(text, msg), (text, rc, msg)
        if "ws" not in kw and "nbytes" not in kw and d is not None:   # the name query refuses the same descriptor with the same message
            assert _names(d).startswith("refused: sd_preprocess_kernel_names") and re.search(text, _names(d)), _names(d)

    refused("null", None)
    for field in ("images", "out", "h_bounds", "h_kk", "v_bounds", "v_kk", "mean3", "std3"):
        refused("null", _desc(**{field: None}))
    refused("null", _desc(), ws=None)
    for shape in (dict(B=0), dict(Hin=0), dict(Win=-1), dict(Hout=0), dict(Wout=0), dict(h_ksize=0), dict(v_ksize=0)):
        refused("bad shape", _desc(**shape))
    refused("geometry", _desc(geometry=7))
    refused("SD_GEOM_WINDOW", _desc(window=P))
    refused("SD_GEOM_WINDOW", _desc("letterbox", window=P))
    refused("null", _desc("window", window=None))
    refused("does not fit", _desc("window", Hout=CANVAS[1] + 1))
    refused("does not lie inside", _desc("letterbox", g1=WOUT))
    refused("fill", _desc("letterbox", fill3=None))
    refused("do not combine", _desc(affine=P, persp=P))
    refused("go together", _desc(jitter_order=P))
    refused("go together", _desc(jitter_factors=P))
    refused("go together", _desc(mosaic_geom=P))
    refused("go together", _desc(mosaic_affine=P))
    for stages, late in ((("affine",), ()), (("mosaic",), ()), ((), ("persp",))):
        refused("fill", _desc(stages=stages, late=late, fill3=None))
    for late in (("jpeg",), ("noise", "jpeg", "tone")):
        refused("16 x 16 MCUs", _desc(late=late, Wout=24, Hout=16))
    for late in (("jpeg",), ("tone",)):
        refused("aligned", _desc(late=late), ws=P + 4)
    assert run(_desc(late=("noise",)), ws=P + 4, nbytes=0)[0] == -2   # noise has no alignment rule: the call gets as far as the size check
    # B is a grid dimension of the jitter, warp, mosaic and late launches, not of the plain resize
    for stages, late in ((("jitter",), ()), (("affine",), ()), (("mosaic",), ()), ((), ("blur",)), ((), ("noise",))):
        refused(r"batch 65536 > 65535", _desc(stages=stages, late=late, B=65536))
    for is_list in (False, True):
        assert not _names(_desc(is_list=is_list, B=65536)).startswith("refused")
        assert run(_desc(is_list=is_list, B=65536), nbytes=0)[0] == -2
    refused("LDS staging buffer", _desc(is_list=True, Win=21835))
    assert not _names(_desc(is_list=True, Win=21834)).startswith("refused")
    assert not _names(_desc(Win=21835)).startswith("refused")        # the packed form stages nothing
    refused("LDS staging buffer", _desc("window", is_list=True, Win=30000, g1=21835))
    assert not _names(_desc("window", is_list=True, Win=30000)).startswith("refused")           # the window's span binds, not Win
    for geometry, is_list, stages, late in CASES[::5]:
        d = _desc(geometry, is_list, stages, late)
        n = lib.sd_preprocess_chain_workspace_bytes(C.byref(d))
        refused(f"workspace {n - 1} < {n}$", d, code=-2, nbytes=n - 1)


def test_chain_workspace_is_the_legacy_size_or_less():
    """The parent's Python layer asked the size query of the highest form whose table was set; the chain's size is never more, and the same
    where no late stage is set.  The legacy queries return what include/sdnet_hip.h states: [horizontal intermediate | image A | grey sums
    | image B | JPEG planes (1.5 bytes per pixel) | tone histograms (3 x 256 uint32 per image)], each a multiple of 256 bytes."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    frame, sums = _align(B * HOUT * WOUT * 3), _align(B * 8)
    planes, hist = _align(B * HOUT * WOUT * 3 // 2), B * 3 * 256 * 4
    stretch_tmp = _align(B * HIN * WOUT * 3)
    assert lib.sd_preprocess_workspace_bytes(B, HIN, WIN, WOUT) == stretch_tmp
    assert lib.sd_preprocess_jitter_workspace_bytes(B, HIN, WIN, HOUT, WOUT) == stretch_tmp + frame + sums
    assert lib.sd_preprocess_affine_workspace_bytes(B, HIN, WIN, HOUT, WOUT) == stretch_tmp + 2 * frame + sums
    assert lib.sd_preprocess_mosaic_workspace_bytes(B, HIN, WIN, HOUT, WOUT) == stretch_tmp + 2 * frame + sums
    assert lib.sd_preprocess_affine_workspace_bytes(2, 8, 8, 4, 4) == lib.sd_preprocess_jitter_workspace_bytes(2, 8, 8, 4, 4) + 256
    for geometry in GEOMETRIES:
        gid, Hg, Wg, g0, g1 = _geometry(geometry)
        tmp = {"stretch": stretch_tmp, "window": _align(B * g0 * WOUT * 3), "letterbox": _align(B * HIN * Wg * 3)}[geometry]
        full = tmp + 2 * frame + sums
        if geometry == "window":
            assert lib.sd_preprocess_window_workspace_bytes(B, g0, HOUT, WOUT) == full
        if geometry == "letterbox":
            assert lib.sd_preprocess_letterbox_workspace_bytes(B, HIN, Wg, HOUT, WOUT) == full
        args = (gid, B, HIN, WIN, Wg, HOUT, WOUT, g0)
        assert lib.sd_preprocess_blur_workspace_bytes(*args) == full
        assert lib.sd_preprocess_jpeg_workspace_bytes(*args) == full + planes
        assert lib.sd_preprocess_tone_workspace_bytes(*args) == lib.sd_preprocess_noise_workspace_bytes(*args) == full + planes + hist
        for geo, is_list, stages, late in CASES:
            if geo != geometry:
                continue
            d = _desc(geometry, is_list, stages, late)
            got = lib.sd_preprocess_chain_workspace_bytes(C.byref(d))
            what = f"{geometry} list={is_list} {stages} {late}"
            if late:
                legacy = full + planes + hist if "noise" in late or "tone" in late else full + planes if "jpeg" in late else full
                assert 0 < got <= legacy, what
                assert got >= (full + planes + hist if "tone" in late else full + planes if "jpeg" in late else full), what
            elif geometry != "stretch" or "mosaic" in stages or "affine" in stages:
                assert got == full, what
            else:
                assert got == (stretch_tmp + frame + sums if "jitter" in stages else stretch_tmp), what
    assert lib.sd_preprocess_chain_workspace_bytes(C.byref(_desc(geometry=7))) == 0             # a refused descriptor has no size
