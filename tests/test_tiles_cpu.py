"""Tiled inference (`--tiles`, `--tile_overlap`), the parts that need no GPU: the flags, the canvas / origin arithmetic, the ramp weight
and owner tables, the exported symbols, the argument validation of `sd_tile_views` / `sd_tile_merge_nms` (host code that runs before any
launch), the decoder's host assembly and the refusals."""
from argparse import Namespace

import numpy as np
import pytest

from tests.tile_ref import axis_tables, canvas_size, tile_weights


def test_tiles_flags_parse_default_to_off_and_reject_bad_values():
    from structuredetector_amd.utils.args import Arguments, check_tile_overlap, parse_tiles
    parser = Arguments().parser
    assert parser.parse_args([]).tiles == "" and parser.parse_args([]).tile_overlap == 64
    ns = parser.parse_args(["--tiles", "3x2", "--tile_overlap", "32"])
    assert ns.tiles == "3x2" and ns.tile_overlap == 32
    assert parse_tiles("") == () and parse_tiles("  ") == () and parse_tiles("1x1") == ()
    assert parse_tiles("2x2") == (2, 2) and parse_tiles("3x2") == (3, 2) and parse_tiles(" 8X1 ") == (8, 1) and parse_tiles("1x8") == (1, 8)
    assert parse_tiles((3, 2)) == (3, 2) and parse_tiles(()) == () and parse_tiles((1, 1)) == ()        # an already finalized namespace
    for garbage in ("abc", "2", "2x", "x2", "2x2x2", "2,2", "2.5x2", "axb"):
        with pytest.raises(ValueError, match="COLUMNSxROWS"):
            parse_tiles(garbage)
    for bad in ("0x2", "2x0", "9x1", "1x9", "-1x2"):
        with pytest.raises(ValueError, match="1 to 8"):
            parse_tiles(bad)
    assert check_tile_overlap(64, 512, 512) == 64 and check_tile_overlap(0, 128, 128) == 0 and check_tile_overlap(64, 128, 256) == 64
    for bad in (16, 48, 65, 63.5):
        with pytest.raises(ValueError, match="multiple of 32"):
            check_tile_overlap(bad, 512, 512)
    for bad, (W, H) in ((96, (128, 128)), (64, (96, 512)), (288, (512, 512)), (-32, (512, 512))):
        with pytest.raises(ValueError, match="half the smaller side"):
            check_tile_overlap(bad, W, H)
    text = " ".join(parser.format_help().split())
    assert "--tiles CxR" in text and "--tile_overlap PX" in text and "--max_objects / --max_parts" in text and "counting images" in text


def test_canvas_and_origin_arithmetic():
    from structuredetector_amd.utils.args import tile_canvas, tile_origins
    assert tile_canvas(512, 512, (2, 2), 64) == (960, 960)
    assert tile_canvas(512, 384, (3, 2), 64) == (1408, 704)
    assert tile_canvas(128, 128, (1, 1), 64) == (128, 128) and tile_canvas(128, 96, (8, 8), 0) == (1024, 768)
    assert tile_origins(512, 384, (3, 2), 64) == [(0, 0), (0, 448), (0, 896), (320, 0), (320, 448), (320, 896)]
    for W, H, grid, O in ((512, 512, (2, 2), 64), (128, 96, (3, 2), 32), (64, 64, (8, 8), 32), (256, 128, (5, 1), 0)):
        Wc, Hc = tile_canvas(W, H, grid, O)
        assert Wc % 32 == 0 and Hc % 32 == 0
        origins = tile_origins(W, H, grid, O)
        assert len(origins) == grid[0] * grid[1] and origins[-1] == (Hc - H, Wc - W)          # the last tile ends at the canvas edge
        assert (Wc, Hc) == (canvas_size(W, grid[0], O), canvas_size(H, grid[1], O))


@pytest.mark.parametrize("n,o,T", [(8, 4, 2), (9, 3, 3), (7, 3, 2), (40, 8, 2), (16, 4, 8), (128, 16, 2), (128, 16, 3), (128, 64, 8), (33, 1, 4),
                                   (10, 5, 3)])
def test_ramp_weights_and_owners(n, o, T):
    hi, l, two, w_lo, w_hi, own, own_l = axis_tables(n, o, T)
    nc = canvas_size(n, T, o)
    assert len(hi) == nc and hi.min() == 0 and hi.max() == T - 1 and (np.diff(hi) >= 0).all()
    assert (l >= 0).all() and (l < n).all() and int(two.sum()) == (T - 1) * o
    lo32, hi32 = w_lo.astype(np.float32), w_hi.astype(np.float32)
    # both weights of every overlap column lie in (0, 1) and sum to 1 within one fp32 ulp (of 1: 2^-23)
    assert (lo32[two] > 0).all() and (lo32[two] < 1).all() and (hi32[two] > 0).all() and (hi32[two] < 1).all()
    assert np.abs(lo32[two].astype(np.float64) + hi32[two].astype(np.float64) - 1.0).max() <= 2.0 ** -23
    # mirroring the canvas swaps the two tiles of a seam: w_lo at l is w_hi at o-1-l, bit for bit
    for s in range(1, T):
        X = np.arange(s * (n - o), s * (n - o) + o)
        assert (two[X]).all() and (hi[X] == s).all()
        assert (lo32[X] == hi32[X][::-1]).all()
        assert (np.diff(hi32[X]) > 0).all()                                # a ramp
    # exactly one owner, a covering tile, the one with the larger weight; the lower tile on a tie (o odd, l = (o-1)/2)
    assert ((own == hi) | (two & (own == hi - 1))).all()
    assert (own_l == np.where(own == hi, l, l + n - o)).all() and (own_l < n).all()
    assert (own[two & (lo32 > hi32)] == hi[two & (lo32 > hi32)] - 1).all() and (own[two & (lo32 < hi32)] == hi[two & (lo32 < hi32)]).all()
    tie = two & (lo32 == hi32)
    assert int(tie.sum()) == ((T - 1) if o % 2 else 0) and (l[tie] == (o - 1) // 2).all() and (own[tie] == hi[tie] - 1).all()
    # outside the overlaps: one tile, weight 1
    assert (w_hi[~two] == 1.0).all() and (w_lo[~two] == 0.0).all()
    # the per-tile view of the same tables: every canvas cell's weights come back
    wt = tile_weights(n, o, T)
    assert wt.shape == (T, n) and (wt > 0).all() and (wt <= 1).all()
    total = np.zeros(nc)
    for t in range(T):
        total[t * (n - o):t * (n - o) + n] += wt[t]
    assert np.abs(total - 1).max() <= 1e-15


@pytest.mark.parametrize("n,o,T", [(8, 0, 1), (8, 4, 1), (16, 0, 2), (16, 0, 8), (7, 0, 3)])
def test_one_tile_and_no_overlap_give_all_ones_tables(n, o, T):
    hi, l, two, w_lo, w_hi, own, own_l = axis_tables(n, o, T)
    assert not two.any() and (w_hi == 1.0).all() and (w_lo == 0.0).all() and (tile_weights(n, o, T) == 1.0).all()
    assert (own == hi).all() and (hi * (n - o) + l == np.arange(canvas_size(n, T, o))).all()


def test_library_exports_the_tile_symbols():
    from structuredetector_amd import _lib as L
    assert {"sd_tile_views", "sd_tile_merge_nms"} <= set(L.declared_symbols())
    assert hasattr(L.lib(), "sd_tile_views") and hasattr(L.lib(), "sd_tile_merge_nms")


def test_tile_entry_points_reject_bad_geometry_without_touching_the_gpu():
    """Both entry points validate before they launch: every bad call returns SD_ERR_INVALID (-1) with a message that names the
    function.  (The pointers are never dereferenced on the device: no call below reaches a launch.)"""
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def views(canvas=16, out=32, B=1, Hc=24, Wc=40, H=16, W=24, Ty=2, Tx=2, O=8):
        return lib.sd_tile_views(canvas, out, B, Hc, Wc, H, W, Ty, Tx, O, 0)

    def merge(hm=16, sb=7 * 64, sc=64, Cc=3, reg=32, r_sb=7 * 64, r_sc=64, R=4, out_hm=48, out_reg=64, B=1, h=8, w=8, Ty=2, Tx=2, o=2):
        return lib.sd_tile_merge_nms(hm, sb, sc, Cc, reg, r_sb, r_sc, R, out_hm, out_reg, B, h, w, Ty, Tx, o, 0)

    view_cases = {"null canvas": dict(canvas=None), "null output": dict(out=None), "B = 0": dict(B=0), "H = 0": dict(H=0), "W = 0": dict(W=0),
                  "Tx = 0": dict(Tx=0), "Tx = 9": dict(Tx=9, Wc=9 * 24 - 8 * 8), "Ty = 0": dict(Ty=0), "Ty = 9": dict(Ty=9, Hc=9 * 16 - 8 * 8),
                  "2O > min(H, W)": dict(O=12, Hc=20, Wc=36), "O < 0": dict(O=-8, Hc=40, Wc=56),
                  "canvas width mismatch": dict(Wc=44), "canvas height mismatch": dict(Hc=32)}
    merge_cases = {"null hm": dict(hm=None), "null out_hm": dict(out_hm=None), "R > 0 with a null reg": dict(reg=None),
                   "R > 0 with a null out_reg": dict(out_reg=None), "R < 0": dict(R=-1), "B = 0": dict(B=0), "C = 0": dict(Cc=0),
                   "h = 0": dict(h=0), "w = 0": dict(w=0), "Tx = 0": dict(Tx=0), "Tx = 9": dict(Tx=9), "Ty = 0": dict(Ty=0), "Ty = 9": dict(Ty=9),
                   "2o > min(h, w)": dict(o=5), "2o > h only": dict(h=8, w=16, o=6, sc=128, sb=7 * 128, r_sc=128, r_sb=7 * 128), "o < 0": dict(o=-1),
                   "channel stride smaller than a plane": dict(sc=63), "batch stride smaller than a plane": dict(sb=63),
                   "regression channel stride smaller than a plane": dict(r_sc=63), "regression batch stride smaller than a plane": dict(r_sb=63)}
    for call, name, cases in ((views, b"sd_tile_views", view_cases), (merge, b"sd_tile_merge_nms", merge_cases)):
        for what, kw in cases.items():
            lib.sd_set_option(b"no_such_option", 1)                        # leaves another message behind: the next one must be this call's
            assert call(**kw) == -1, what
            assert name in lib.sd_last_error(), f"{what}: {lib.sd_last_error()}"
    assert views(Wc=44) == -1 and b"40 x 24" in lib.sd_last_error()
    assert merge(o=5) == -1 and b"overlap" in lib.sd_last_error()


def _args(**kw):
    from tests.test_host_cpu import make_args
    return make_args(2, 1, 4, 6, **kw)


def test_tiled_decoder_reports_network_input_pixels():
    """The host assembly on a hand-made packed result: a 2 x 2 grid of 32 x 32-cell tiles with an overlap of 8 cells is a 56 x 56 map of
    a 128 x 128 network input -- cell * 128 / 56 on both axes; a 3 x 1 grid of 32 x 16 (w x h) tiles is 80 x 16 cells of 128 x 64."""
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data import FusedOutputDecoder, TiledOutputDecoder
    args = _args()
    K, P = 4, 6
    host = {"anchor_out": np.zeros((1, K, 4), np.float32), "part_out": np.zeros((1, P, 6), np.float32), "assign": np.full((1, P), -1, np.int32)}
    host["anchor_out"][0, 0] = (28.0, 14.0, 0.9, 1)
    host["anchor_out"][0, 1] = (55.5, 3.25, 0.8, 0)
    host["anchor_out"][0, 2] = (1.0, 1.0, 0.2, 0)                                     # below the threshold
    host["part_out"][0, 0, :4] = (30.0, 15.0, 0.7, 0)
    host["part_out"][0, 1, :4] = (50.0, 5.0, 0.6, 0)
    host["assign"][0, :2] = (0, 1)
    dec = TiledOutputDecoder(args, (2, 2), 8)
    assert dec.tile_map(56, 56) == (32, 32) and dec._input_size(56, 56) == (128, 128) and dec._linkage_side(56, 56) == 32
    anns, raws = dec._assemble(host, 1, 56, 56, 0.5, True)
    sx = 128 / 56
    got = [(o.name, o.x, o.y, o.anchor.score, [(p.kind, p.x, p.y) for p in o.parts]) for o in anns[0].objects]
    assert got == [("label1", 28.0 * sx, 14.0 * sx, float(np.float32(0.9)), [("part0", 30.0 * sx, 15.0 * sx)]),
                   ("label0", 55.5 * sx, 3.25 * sx, float(np.float32(0.8)), [("part0", 50.0 * sx, 5.0 * sx)])]
    assert [(p.x, p.y) for p in raws[0]] == [(30.0 * sx, 15.0 * sx), (50.0 * sx, 5.0 * sx)]
    wide = TiledOutputDecoder(args, (3, 1), 8)
    assert wide.tile_map(16, 80) == (16, 32) and wide._input_size(16, 80) == (64, 128) and wide._linkage_side(16, 80) == 16
    anns, _ = wide._assemble(host, 1, 16, 80, 0.5, False)
    assert (anns[0].objects[0].x, anns[0].objects[0].y) == (28.0 * (128 / 80), 14.0 * (64 / 16))
    # the plain decoders are unchanged: cell * down_ratio
    plain, _ = FusedOutputDecoder(args)._assemble(host, 1, 56, 56, 0.5, False)
    assert (plain[0].objects[0].x, plain[0].objects[0].y) == (112.0, 56.0)
    with pytest.raises(L.SdError, match="not 2 x 2 tiles"):
        dec.tile_map(57, 56)


def test_tiles_refuse_flip_and_scale_tta_and_synthetic():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.cli.evaluate import refuse_synthetic_resampling
    from structuredetector_amd.model.tta import with_tta
    for kw in (dict(tta="hflip"), dict(tta_scales="0.75,1.25"), dict(tta="hvflip", tta_scales=(0.75,))):
        args = _args(width=128, height=128, tiles="2x2", tile_overlap=32, **kw)
        with pytest.raises(L.SdError, match="--tiles does not combine with --tta / --tta_scales"):
            with_tta("net", "decoder", args)
    # off: the previous code path, whatever the overlap says
    for tiles in ("", "1x1", ()):
        assert with_tta("net", "decoder", _args(width=128, height=128, tiles=tiles, tile_overlap=48)) == ("net", "decoder")
    assert with_tta("net", "decoder", _args(width=128, height=128)) == ("net", "decoder")
    # on: the net behind TiledNet, with its decoder; a bad overlap is refused there as well
    from structuredetector_amd.data import TiledOutputDecoder
    from structuredetector_amd.model.tiles import TiledNet
    net, dec = with_tta("net", "decoder", _args(width=128, height=96, tiles="3x2", tile_overlap=32))
    assert isinstance(net, TiledNet) and net.needs_sources and net.grid == (3, 2) and net.canvas == (320, 160) and net.overlap_cells == 8
    assert isinstance(dec, TiledOutputDecoder) and dec.grid == (3, 2) and dec.overlap_cells == 8
    for overlap in (48, 96):
        with pytest.raises(L.SdError, match="tile_overlap"):
            with_tta("net", "decoder", _args(width=128, height=128, tiles="2x2", tile_overlap=overlap))
    with pytest.raises(SystemExit, match="source image"):
        refuse_synthetic_resampling(Namespace(synthetic=8, tiles=(2, 2), tta_scales=()))
    refuse_synthetic_resampling(Namespace(synthetic=0, tiles=(2, 2), tta_scales=()))
    refuse_synthetic_resampling(Namespace(synthetic=8, tiles=(), tta_scales=()))
