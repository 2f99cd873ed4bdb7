"""Cross-label anchor suppression (`--label_nms`), the parts that need no GPU: the flag, the exported symbols, the argument validation of
`sd_label_nms` (host code that runs before any launch), how `with_tta` composes `LabelNms` with the other wrappers,
and the definition's helpers (tests/label_nms_ref.py) against each other."""
import numpy as np
import pytest
import torch

from tests.label_nms_ref import cpu_nms5, expected_label_nms, loop_label_nms, normal_logits, tie_logits


def test_label_nms_flag_parses_defaults_to_off_and_rejects_bad_values():
    from structuredetector_amd.utils.args import Arguments, check_label_nms
    parser = Arguments().parser
    assert parser.parse_args([]).label_nms == 0
    assert parser.parse_args(["--label_nms", "3"]).label_nms == 3
    with pytest.raises(SystemExit):
        parser.parse_args(["--label_nms", "2.5"])
    assert [check_label_nms(r) for r in (0, 1, 2, 8, 4.0)] == [0, 1, 2, 8, 4]
    assert type(check_label_nms(4.0)) is int
    for bad in (-1, 9, 100):
        with pytest.raises(ValueError, match=r"\[0, 8\]"):
            check_label_nms(bad)
    for bad in (1.5, True):
        with pytest.raises(ValueError, match="integer"):
            check_label_nms(bad)
    text = " ".join(parser.format_help().split())
    assert "--label_nms R" in text and "Not consulted by train" in text


def test_library_exports_the_label_nms_symbol():
    from structuredetector_amd import _lib as L
    assert "sd_label_nms" in L.declared_symbols() and hasattr(L.lib(), "sd_label_nms")


def test_label_nms_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    """The entry point validates before it launches: every bad call returns SD_ERR_INVALID (-1) with a message that names the function.
    (The pointers are never dereferenced on the device: no call below reaches a launch.)"""
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def maps(p=16, sb=3 * 64, sc=64, out=32, B=1, M=3, h=8, w=8, R=2):
        return lib.sd_label_nms(p, sb, sc, out, B, M, h, w, R, 0)

    cases = {"null input": dict(p=None), "null output": dict(out=None), "R = 0": dict(R=0), "R = 9": dict(R=9), "R < 0": dict(R=-1),
             "M = 0": dict(M=0), "M < 0": dict(M=-2), "M = 257": dict(M=257, sb=257 * 64), "B = 0": dict(B=0), "h = 0": dict(h=0), "w = 0": dict(w=0),
             "channel stride below a plane": dict(sc=63), "batch stride below a plane": dict(sb=63), "B beyond the grid": dict(B=65536),
             "M*h*w = 2^31": dict(M=128, h=4096, w=4096, sc=1 << 24, sb=1 << 31)}
    for what, kw in cases.items():
        lib.sd_set_option(b"no_such_option", 1)                            # leaves another message behind: the next one must be this call's
        assert maps(**kw) == -1, what
        assert b"sd_label_nms" in lib.sd_last_error(), f"{what}: {lib.sd_last_error()}"
    assert maps(R=9) == -1 and b"R=9" in lib.sd_last_error()
    assert maps(M=257, sb=257 * 64) == -1 and b"M=257" in lib.sd_last_error()


def _args(**kw):
    from tests.test_host_cpu import make_args
    return make_args(2, 1, 4, 6, **kw)


def test_with_tta_applies_label_nms_last_and_off_is_the_present_path():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import FusedOutputDecoder, TiledOutputDecoder
    from structuredetector_amd.model.label_nms import LabelNms
    from structuredetector_amd.model.tiles import TiledNet
    from structuredetector_amd.model.tta import FlipTta, ScaleTta, TransposeTta, with_tta
    # off: the identical objects, with and without the attribute
    for kw in ({}, dict(label_nms=0)):
        net, dec = with_tta("net", "decoder", _args(width=128, height=128, **kw))
        assert net == "net" and dec == "decoder"
    for kw, inner in ((dict(tta="hflip"), FlipTta), (dict(tta_scales="0.75"), ScaleTta), (dict(tta_transpose=True), TransposeTta),
                      (dict(tiles="2x2", tile_overlap=32), TiledNet)):
        net, dec = with_tta("net", "decoder", _args(width=128, height=128, label_nms=0, **kw))
        assert type(net) is inner
    # on: LabelNms around each, with the inner path's decoder class
    cases = ((dict(), str, FusedOutputDecoder, False), (dict(tta="hvflip"), FlipTta, FusedOutputDecoder, False),
             (dict(tta_scales="0.75,1.25", tta="hflip"), ScaleTta, FusedOutputDecoder, True),
             (dict(tta_transpose=True), TransposeTta, FusedOutputDecoder, False),
             (dict(tiles="3x2", tile_overlap=32), TiledNet, TiledOutputDecoder, True))
    for kw, inner, decoder, sources in cases:
        net, dec = with_tta("net", "decoder", _args(width=128, height=128, label_nms=3, **kw))
        assert type(net) is LabelNms and net.R == 3 and type(net.net) is inner and type(dec) is decoder, kw
        assert net.needs_sources is sources and (inner is str or net.net.net == "net")
    net, dec = with_tta("net", "decoder", _args(width=128, height=128, label_nms=2, tiles="3x2", tile_overlap=32))
    assert dec.grid == (3, 2) and dec.overlap_cells == 8
    # the refusals and their texts are unchanged
    with pytest.raises(L.SdError, match="--tiles does not combine with --tta / --tta_scales"):
        with_tta("net", "decoder", _args(width=128, height=128, label_nms=2, tiles="2x2", tile_overlap=32, tta="hflip"))
    with pytest.raises(L.SdError, match="--tta_transpose does not combine with --tta_scales / --tiles"):
        with_tta("net", "decoder", _args(width=128, height=128, label_nms=2, tta_transpose=True, tta_scales="0.75"))
    for bad in (9, -1, 2.5):
        with pytest.raises(L.SdError, match="radius of 1 .. 8"):
            LabelNms("net", _args(), bad)


def _maps(shape, seed, family):
    """Suppressed probability maps made on the CPU: the 5x5 rule on torch's sigmoid of a logit family."""
    x = tie_logits(shape, seed) if family == "tie" else normal_logits(shape, seed)
    return cpu_nms5(torch.sigmoid(x).clamp(1e-6, 1 - 1e-6))


@pytest.mark.parametrize("family", ["tie", "normal"])
@pytest.mark.parametrize("B,M,h,w,R", [(2, 3, 7, 9, 2), (1, 5, 17, 19, 8)])
def test_pooled_helper_equals_the_loop_helper(B, M, h, w, R, family):
    P = _maps((B, M, h, w), 11 * M + R, family)
    got = expected_label_nms(P, R).numpy()
    want = loop_label_nms(P.numpy(), R)
    assert got.tobytes() == want.tobytes()
    peaks, kept = int((P > 0).sum()), int((got > 0).sum())
    assert 0 < kept < peaks                                                # something is suppressed, something survives
    if family == "tie":                                                    # and the lowest-label rule decides somewhere
        best = P.max(1).values
        assert int((((P == best[:, None]) & (best[:, None] > 0)).sum(1) > 1).sum()) > 0


@pytest.mark.parametrize("R", [1, 2])
def test_one_label_within_the_5x5_window_is_the_identity(R):
    for family in ("tie", "normal"):
        P = _maps((2, 1, 16, 16), 5, family)
        assert torch.equal(expected_label_nms(P, R), P)
        assert loop_label_nms(P.numpy(), R).tobytes() == P.numpy().tobytes()


def test_one_label_with_a_wider_window_thins_its_own_peaks():
    P = _maps((1, 1, 16, 16), 5, "normal")
    out = expected_label_nms(P, 4)
    assert not torch.equal(out, P)
    assert 0 < int((out > 0).sum()) < int((P > 0).sum())
    assert torch.equal(out[out > 0], P[out > 0])                           # survivors keep their value
    assert loop_label_nms(P.numpy(), 4).tobytes() == out.numpy().tobytes()


def test_consequences_on_planted_peaks():
    """Two labels k cells apart keep only the higher for k <= R and both for k = R + 1; equal values at one cell keep the lower label;
    equal values at two cells within R keep both; a corner peak sees no padding."""
    R = 2
    for k in (1, 2, 3):
        P = torch.zeros(1, 2, 9, 12)
        P[0, 1, 4, 3], P[0, 0, 4, 3 + k] = 0.9, 0.8
        out = expected_label_nms(P, R)
        assert out[0, 1, 4, 3] == 0.9 and (out[0, 0, 4, 3 + k] == 0.8) == (k == R + 1)
    P = torch.zeros(1, 3, 9, 12)
    P[0, 1, 4, 4] = P[0, 2, 4, 4] = 0.7
    out = expected_label_nms(P, R)
    assert out[0, 1, 4, 4] == 0.7 and out[0, 2, 4, 4] == 0 and int((out > 0).sum()) == 1
    P = torch.zeros(1, 2, 9, 12)
    P[0, 0, 4, 4] = P[0, 1, 5, 6] = 0.6
    assert torch.equal(expected_label_nms(P, R), P)
    P = torch.zeros(1, 2, 9, 12)
    P[0, 1, 0, 0] = P[0, 0, 8, 11] = 1e-6
    assert torch.equal(expected_label_nms(P, 8), P)
    assert np.array_equal(loop_label_nms(P.numpy(), 8), P.numpy())
