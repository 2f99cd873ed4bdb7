"""Transposed views (`--tta_transpose`, `--aug_transpose`), the parts that need no GPU: the flags, the exported symbols, the argument
validation of `sd_d4_views` / `sd_d4_merge_nms` / `sd_transpose_select` (host code that runs before any launch), the annotation rule, the
`with_tta` refusals and the extra training draw."""
import ctypes as C
from argparse import Namespace

import pytest
import torch


def test_flags_parse_and_default_to_off():
    from structuredetector_amd.utils.args import Arguments
    parser = Arguments().parser
    ns = parser.parse_args([])
    assert ns.tta_transpose is False and ns.aug_transpose == 0.0
    ns = parser.parse_args(["--tta_transpose", "--tta", "hvflip", "--aug_transpose", "0.25"])
    assert ns.tta_transpose is True and ns.tta == "hvflip" and ns.aug_transpose == 0.25
    text = " ".join(parser.format_help().split())
    assert "--tta_transpose" in text and "2x the views" in text and "Combines with --tta" in text and "--aug_transpose P" in text
    assert "--tta {none,hflip,vflip,hvflip}" in text                              # the flip choices are as they were


def test_aug_transpose_range_and_square_rule():
    from structuredetector_amd.utils.args import Arguments, check_aug_transpose
    for bad in ("-0.1", "1.5"):
        with pytest.raises(AssertionError, match="aug_transpose"):
            Arguments().parse(["--aug_transpose", bad])
    parser = Arguments().parser
    assert check_aug_transpose(parser.parse_args(["--aug_transpose", "0.5", "-W", "128", "-H", "128"])) == 0.5
    assert check_aug_transpose(parser.parse_args(["-W", "128", "-H", "96"])) == 0.0          # off: any shape
    with pytest.raises(ValueError, match="square network input, not 128 x 96"):
        check_aug_transpose(parser.parse_args(["--aug_transpose", "0.5", "-W", "128", "-H", "96"]))
    from structuredetector_amd.model.trainer import Trainer
    with pytest.raises(ValueError, match="square network input"):                  # `train` checks before it builds anything (no GPU is touched)
        Trainer(parser.parse_args(["--aug_transpose", "0.5", "-W", "128", "-H", "96", "--train_dir", "x"]))


def test_library_exports_the_three_symbols():
    from structuredetector_amd import _lib as L
    handle = L.lib()
    names = {"sd_d4_views", "sd_d4_merge_nms", "sd_transpose_select"}
    assert names <= set(L.declared_symbols())
    assert all(hasattr(handle, n) for n in names)


def _flips(*values):
    return (C.c_ubyte * len(values))(*values)


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """All three entry points validate before they launch: every bad call returns SD_ERR_INVALID (-1) and sd_last_error() names the function.
    (The pointers are never dereferenced: no call below reaches a launch.)"""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    ok2 = _flips(0, 1)

    def views(x=16, out=1 << 20, out_t=2 << 20, B=1, H=32, W=32, V=2, flips=ok2):
        return lib.sd_d4_views(x, out, out_t, B, H, W, V, flips, 0)

    def merge(hm=16, sb=7 * 64, sc=64, hm_t=1 << 20, sb_t=7 * 64, sc_t=64, out=2 << 20, B=1, Cc=3, h=8, w=8, V=2, flips=ok2):
        return lib.sd_d4_merge_nms(hm, sb, sc, hm_t, sb_t, sc_t, out, B, Cc, h, w, V, flips, 0)

    def select(x=16, out=1 << 20, B=2, P=3, S=8, sel=64):
        return lib.sd_transpose_select(x, out, B, P, S, sel, 0)

    def expect(call, name, what, **kw):
        lib.sd_set_option(b"no_such_option", 1)                            # leaves another message behind: the next one must be this call's
        assert call(**kw) == -1, f"{name.decode()}: {what}"
        assert name in lib.sd_last_error(), f"{name.decode()}: {what}: {lib.sd_last_error()}"

    for call, name in ((views, b"sd_d4_views"), (merge, b"sd_d4_merge_nms")):
        first = "x" if call is views else "hm"
        second = "out_t" if call is views else "hm_t"
        cases = {"Vf = 3": dict(V=3, flips=_flips(0, 1, 2)), "Vf = 8": dict(V=8, flips=_flips(*[0] * 8)), "Vf = 0": dict(V=0),
                 "view 0 flipped (Vf = 1)": dict(V=1, flips=_flips(1)), "view 0 flipped (Vf = 2)": dict(flips=_flips(1, 0)),
                 "view 0 flipped (Vf = 4)": dict(V=4, flips=_flips(3, 1, 2, 0)), "flip byte of 4": dict(flips=_flips(0, 4)),
                 "null input": {first: None}, "null transposed": {second: None}, "null output": dict(out=None), "null view_flips": dict(flips=None),
                 "h = 0": {"H" if call is views else "h": 0}, "h < 0": {"H" if call is views else "h": -8},
                 "w = 0": {"W" if call is views else "w": 0}, "w < 0": {"W" if call is views else "w": -1}, "B = 0": dict(B=0), "B < 0": dict(B=-2)}
        for what, kw in cases.items():
            expect(call, name, what, **kw)
    expect(views, b"sd_d4_views", "3*H*W >= 2^31", H=1 << 15, W=1 << 15)
    expect(merge, b"sd_d4_merge_nms", "C = 0", Cc=0)
    expect(merge, b"sd_d4_merge_nms", "C*h*w >= 2^31", Cc=8, h=1 << 14, w=1 << 14, sb=1 << 40, sc=1 << 30, sb_t=1 << 40, sc_t=1 << 30)
    expect(merge, b"sd_d4_merge_nms", "C beyond the grid", Cc=70000, sb=1 << 30, sb_t=1 << 30)
    for kw in (dict(sc=63), dict(sb=8, B=2), dict(sc_t=63), dict(sb_t=8, B=2)):       # a stride smaller than a plane, on either map
        expect(merge, b"sd_d4_merge_nms", str(kw), **kw)
        assert b"strides" in lib.sd_last_error()
    n = 2 * 3 * 8 * 8 * 4                                                              # bytes of the (2, 3, 8, 8) batch
    cases = {"null input": dict(x=None), "null output": dict(out=None), "null table": dict(sel=None), "B = 0": dict(B=0), "P = 0": dict(P=0),
             "S = 0": dict(S=0), "S < 0": dict(S=-4), "P*S*S >= 2^31": dict(P=8, S=1 << 14),
             "in place": dict(x=4096, out=4096), "out inside x": dict(x=4096, out=4096 + n - 4), "x inside out": dict(x=4096 + n - 4, out=4096)}
    for what, kw in cases.items():
        expect(select, b"sd_transpose_select", what, **kw)
    expect(select, b"sd_transpose_select", "overlap", x=4096, out=4096 + 16)
    assert b"overlap" in lib.sd_last_error()


def _annotation():
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    from structuredetector_amd.utils.types import Box
    objs = [Object("bean", Keypoint("stem", 10.0, 3.5), [Keypoint("leaf", 0.0, 63.0), Keypoint("leaf", 95.0, 7.25)]),
            Object("maize", Keypoint("stem", 40.0, 40.0), [])]
    objs[0].box = Box(2.0, 1.0, 30.5, 9.0)
    return ImageAnnotation("a.png", objs)


def _rows(ann):
    return [(o.name, o.x, o.y, [(p.kind, p.x, p.y) for p in o.parts],
             None if o.box is None else (o.box.x_min, o.box.y_min, o.box.x_max, o.box.y_max)) for o in ann.objects]


def test_transpose_annotation_is_an_involution_and_swaps_the_flips():
    from structuredetector_amd.utils.misc import hflip_annotation, transpose_annotation, vflip_annotation
    W, H = 96, 64
    base = _rows(_annotation())
    once = transpose_annotation(_annotation(), (W, H))
    assert _rows(once)[0][1:3] == (3.5, 10.0) and _rows(once)[0][3][0] == ("leaf", 63.0, 0.0)
    assert _rows(once)[0][4] == (1.0, 2.0, 9.0, 30.5)                              # the box swaps its axes, corners stay ordered
    assert _rows(transpose_annotation(once, (H, W))) == base
    # transpose o hflip = vflip o transpose (the transposed frame is H wide and W high), and the same with the flips exchanged
    a = transpose_annotation(hflip_annotation(_annotation(), (W, H)), (W, H))
    b = vflip_annotation(transpose_annotation(_annotation(), (W, H)), (H, W))
    assert _rows(a) == _rows(b) and _rows(a) != _rows(once)
    a = transpose_annotation(vflip_annotation(_annotation(), (W, H)), (W, H))
    b = hflip_annotation(transpose_annotation(_annotation(), (W, H)), (H, W))
    assert _rows(a) == _rows(b)


def test_with_tta_routes_tta_transpose_and_refuses_the_two_combinations():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import FusedOutputDecoder
    from structuredetector_amd.model.tta import MODES, VIEW_FLIPS, TransposeTta, with_tta
    from tests.test_host_cpu import make_args
    assert VIEW_FLIPS == {"hflip": (0, 1), "vflip": (0, 2), "hvflip": (0, 1, 2, 3)} and MODES == ("none", "hflip", "vflip", "hvflip")
    net, dec = object(), object()
    for mode, flips in (("none", (0,)), ("hflip", (0, 1)), ("hvflip", (0, 1, 2, 3))):
        args = make_args(2, 1, 20, 40, width=128, height=96, tta=mode, tta_transpose=True)
        got, got_dec = with_tta(net, dec, args)
        assert isinstance(got, TransposeTta) and got.net is net and got.flips == flips and isinstance(got_dec, FusedOutputDecoder)
        assert not getattr(got, "needs_sources", False)
    with pytest.raises(L.SdError, match="--tta_transpose does not combine with --tta_scales / --tiles"):
        with_tta(net, dec, make_args(2, 1, 20, 40, width=128, height=128, tta_transpose=True, tta_scales="0.75"))
    with pytest.raises(L.SdError, match="--tta_transpose does not combine with --tta_scales / --tiles"):
        with_tta(net, dec, make_args(2, 1, 20, 40, width=128, height=128, tta_transpose=True, tiles="2x2"))
    assert with_tta(net, dec, make_args(2, 1, 20, 40, width=128, height=128, tta_transpose=False)) == (net, dec)
    with pytest.raises(L.SdError, match="unknown test-time augmentation mode"):
        TransposeTta(net, make_args(2, 1, 20, 40), "rot90")


def test_transpose_draws_are_one_more_draw_and_none_with_the_flag_off():
    from structuredetector_amd.data.augment import TrainAugmentation, ValidationAugmentation
    groups = [[0, 1, 2], [3, 4, 5]]
    common = dict(width=128, height=128, no_augmentation=False, aug_scale=0.2, aug_mosaic=0.5, train_tiles="2x2", tile_overlap=32)

    def batch(aug):
        return aug.draws_for(6), aug.affine_draws_for(6), aug.mosaic_draws_for(6, groups), aug.window_draws_for(6)

    torch.manual_seed(5)
    before = batch(TrainAugmentation(Namespace(**common)))                      # a batch's draws without the attribute
    state = torch.get_rng_state()
    for extra in (dict(aug_transpose=0.0), dict(aug_transpose=0)):
        aug = TrainAugmentation(Namespace(**common, **extra))
        torch.manual_seed(5)
        assert batch(aug) == before
        assert aug.transpose_draws_for(6) is None and torch.equal(torch.get_rng_state(), state)
    # on: the earlier draws are unchanged, then exactly rand(n) in float64
    aug = TrainAugmentation(Namespace(**common, aug_transpose=0.5))
    torch.manual_seed(5)
    assert batch(aug) == before
    u = torch.rand(6, dtype=torch.float64)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    batch(aug)
    bits = aug.transpose_draws_for(6)
    assert torch.equal(torch.get_rng_state(), after)
    assert bits == [int(v < 0.5) for v in u.tolist()] and 0 < sum(bits) < 6
    always = TrainAugmentation(Namespace(**common, aug_transpose=1.0))
    assert always.transpose_draws_for(7) == [1] * 7
    quiet = TrainAugmentation(Namespace(**{**common, "no_augmentation": True}, aug_transpose=1.0))
    state = torch.get_rng_state()
    assert quiet.transpose_draws_for(3) is None and torch.equal(torch.get_rng_state(), state)
    val = ValidationAugmentation(Namespace(width=128, height=128, aug_transpose=1.0))
    assert val.transpose_draws_for(3) is None and torch.equal(torch.get_rng_state(), state)
