"""Flip test-time augmentation (`--tta`), the parts that need no GPU: the flag, the view table, the exported symbols and the argument
validation of `sd_tta_views` / `sd_tta_merge_nms` (host code that runs before any launch)."""
import ctypes as C

import pytest


def test_tta_flag_parses_defaults_to_none_and_rejects_unknown_modes(capsys):
    from structuredetector_amd.utils.args import Arguments
    parser = Arguments().parser
    assert parser.parse_args([]).tta == "none"
    for mode in ("none", "hflip", "vflip", "hvflip"):
        assert parser.parse_args(["--tta", mode]).tta == mode
    with pytest.raises(SystemExit):
        parser.parse_args(["--tta", "rot90"])
    assert "--tta" in capsys.readouterr().err
    text = " ".join(parser.format_help().split())
    assert "--tta {none,hflip,vflip,hvflip}" in text and "Not consulted by train" in text


def test_view_flips_table():
    from structuredetector_amd.model.tta import VIEW_FLIPS
    assert VIEW_FLIPS == {"hflip": (0, 1), "vflip": (0, 2), "hvflip": (0, 1, 2, 3)}
    assert all(flips[0] == 0 and len(flips) in (2, 4) for flips in VIEW_FLIPS.values())          # what the C ABI accepts


def test_library_exports_both_tta_symbols():
    from structuredetector_amd import _lib as L
    handle = L.lib()
    assert {"sd_tta_views", "sd_tta_merge_nms"} <= set(L.declared_symbols())
    assert hasattr(handle, "sd_tta_views") and hasattr(handle, "sd_tta_merge_nms")


def _flips(*values):
    return (C.c_ubyte * len(values))(*values)


def test_tta_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """Both entry points validate before they launch: every bad call returns SD_ERR_INVALID (-1) and sd_last_error() names the function.
    (The pointers are never dereferenced on the device: no call below reaches a launch.)"""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    ok2 = _flips(0, 1)

    def views(x=16, out=32, B=1, H=32, W=32, V=2, flips=ok2):
        return lib.sd_tta_views(x, out, B, H, W, V, flips, 0)

    def merge(hm=16, sb=7 * 64, sc=64, out=32, B=1, Cc=3, h=8, w=8, V=2, flips=ok2):
        return lib.sd_tta_merge_nms(hm, sb, sc, out, B, Cc, h, w, V, flips, 0)

    for call, name in ((views, b"sd_tta_views"), (merge, b"sd_tta_merge_nms")):
        cases = {"V = 3": dict(V=3, flips=_flips(0, 1, 2)), "V = 1": dict(V=1, flips=_flips(0)), "V = 8": dict(V=8, flips=_flips(*[0] * 8)),
                 "view 0 flipped (V = 2)": dict(flips=_flips(1, 0)), "view 0 flipped (V = 4)": dict(V=4, flips=_flips(3, 1, 2, 0)),
                 "flip byte out of range": dict(flips=_flips(0, 4)),
                 "null input": dict(**{"x" if call is views else "hm": None}), "null output": dict(out=None), "null view_flips": dict(flips=None),
                 "h = 0": dict(**{"H" if call is views else "h": 0}), "h < 0": dict(**{"H" if call is views else "h": -8}),
                 "w = 0": dict(**{"W" if call is views else "w": 0}), "B = 0": dict(B=0)}
        for what, kw in cases.items():
            lib.sd_set_option(b"no_such_option", 1)                        # leaves another message behind: the next one must be this call's
            assert call(**kw) == -1, f"{name.decode()}: {what}"
            assert name in lib.sd_last_error(), f"{name.decode()}: {what}: {lib.sd_last_error()}"
    assert merge(Cc=0) == -1 and b"sd_tta_merge_nms" in lib.sd_last_error()
    assert merge(sc=63) == -1 and b"strides" in lib.sd_last_error()       # channel stride smaller than a plane
    assert merge(sb=8, B=2) == -1 and b"strides" in lib.sd_last_error()
