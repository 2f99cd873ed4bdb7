"""`evaluate --pr_curve`, the parts that need no GPU: the prefix property the one-pass sweep rests on (against the Evaluator's own
matching), the binning, AP / best F1 on hand-computed curves, merge, the CSV, the flags and `sd_eval_match`'s argument validation."""
import math

import numpy as np
import pytest

from tests import pr_curve_ref as R


def curve_of(args, case, thresholds=None, images=None):
    """A PrCurve fed with the REFERENCE records of a case (no device)."""
    from structuredetector_amd.model.pr_curve import PrCurve
    curve = PrCurve(args, thresholds)
    match, dist = R.match_ref(case)
    a, p = case["a_list"], case["p_list"]
    sel = slice(None) if images is None else images
    B, K = a.shape[0], a.shape[1]
    off = case["gt_off"]
    idx = np.arange(B)[sel]
    a_gt = np.concatenate([case["gt_cls"][off[b]:off[b + 1]] for b in idx] + [np.zeros(0, np.int32)])
    p_gt = np.concatenate([case["gt_cls"][off[B + b]:off[B + b + 1]] for b in idx] + [np.zeros(0, np.int32)])
    curve.add_records("anchor", a[sel, :, 2], a[sel, :, 3], match[sel, :K], dist[sel, :K], case["side"][sel], a_gt)
    curve.add_records("part", p[sel, :, 2], p[sel, :, 3], match[sel, K:], dist[sel, K:], case["side"][sel], p_gt)
    curve.images += len(idx)
    return curve


def test_prefix_property_against_the_evaluator():
    """Random score-descending lists with tied scores, K = 1 .. 40, 0 .. 12 objects: for EVERY grid threshold and both compare rules the
    one-pass records binned by score give exactly the tp / ndet / npos that Evaluator.eval_anchor / eval_part compute on the prediction
    filtered at that threshold -- by the reference's loop over thresholds and by PrCurve's searchsorted binning alike."""
    from structuredetector_amd.model import Evaluator
    from structuredetector_amd.model.pr_curve import PrCurve, default_grid
    args = R.make_args(parts=("leaf", "ear"))
    rng = np.random.default_rng(20261019)
    grid = default_grid(args.conf_threshold)
    assert len(grid) == 99 and 0.25 in grid and 0.5 in grid                     # thresholds that equal tied fp32 scores exactly
    ev = Evaluator(args)
    checked = 0
    for trial in range(24):
        K, P, G = int(rng.integers(1, 41)), int(rng.integers(1, 41)), int(rng.integers(0, 13))
        case = R.random_case(rng, args, 1, K, P, G)
        match, dist = R.match_ref(case)
        a, p = case["a_list"], case["p_list"]
        ann = case["annotations"][0]
        ref_a = R.counts_ref("anchor", a[..., 2], a[..., 3], match[:, :K], dist[:, :K], case["side"], grid, 2)
        ref_p = R.counts_ref("part", p[..., 2], p[..., 3], match[:, K:], dist[:, K:], case["side"], grid, 2)
        curve = curve_of(args, case)
        for k, t in enumerate(grid):
            pred, raw = R.filtered_prediction(args, case, 0, t)
            want_a, want_p = ev.eval_anchor(pred, ann), ev.eval_part(ann, raw)
            got = curve.at(t)
            for c, name in enumerate(args.labels):
                w = want_a[name]
                assert (ref_a[0][c, k], ref_a[1][c, k]) == (w.tp, w.ndet), (trial, t, name)
                assert (got[name].tp, got[name].npos, got[name].ndet) == (w.tp, w.npos, w.ndet), (trial, t, name)
                if w.tp:
                    assert abs(got[name].avg_acc - np.mean(w.acc)) <= 1e-12
                checked += 1
            for c, name in enumerate(args.parts):
                w = want_p[name]
                assert (ref_p[0][c, k], ref_p[1][c, k]) == (w.tp, w.ndet), (trial, t, name)
                assert (got[name].tp, got[name].npos, got[name].ndet) == (w.tp, w.npos, w.ndet), (trial, t, name)
                checked += 1
    assert checked == 24 * 99 * 4
    # the asymmetry at a threshold that equals a score: the anchor is excluded, the part included
    one = R.random_case(np.random.default_rng(1), args, 1, 1, 1, 1)
    one["a_list"][0, 0, 2] = one["p_list"][0, 0, 2] = 0.5
    got = curve_of(args, one).at(0.5)
    assert sum(got[n].ndet for n in args.labels) == 0 and sum(got[n].ndet for n in args.parts) == 1


def test_ground_truth_tables_match_the_reference():
    from structuredetector_amd.model.pr_curve import PrCurve
    args = R.make_args()
    case = R.random_case(np.random.default_rng(3), args, 3, 4, 5, 6)
    xy, cls, off, img, side = PrCurve(args).ground_truth_tables(case["annotations"])
    for got, want in ((xy, case["gt_xy"]), (cls, case["gt_cls"]), (off, case["gt_off"]), (img, case["img"]), (side, case["side"])):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    empty = PrCurve(args).ground_truth_tables([a for a in R.random_case(np.random.default_rng(3), args, 2, 1, 1, 0)["annotations"]])
    assert empty[0].shape == (0, 2) and empty[2].tolist() == [0, 0, 0, 0, 0]


def hand_curve(args, thresholds, rows, npos):
    """A curve of label 'bean' from (score, hit) rows, ground truths given by count."""
    from structuredetector_amd.model.pr_curve import PrCurve
    curve = PrCurve(args, thresholds)
    n = len(rows)
    score = np.asarray([[r[0] for r in rows]], np.float32).reshape(1, n)
    match = np.asarray([[0 if r[1] else -1 for r in rows]], np.int32).reshape(1, n)
    curve.add_records("anchor", score, np.zeros((1, n)), match, np.full((1, n), 2.0), np.asarray([100.0]), np.zeros(npos, np.int32))
    return curve


def test_ap_and_best_f1_on_hand_computed_curves():
    args = R.make_args()
    grid = [0.1, 0.3, 0.5, 0.7, 0.9]
    # all hits: four detections at 0.8 / 0.6 / 0.4 / 0.2, four ground truths -> precision 1 everywhere, recall 0, 1/4, 2/4, 3/4, 4/4
    c = hand_curve(args, grid, [(0.8, 1), (0.6, 1), (0.4, 1), (0.2, 1)], 4)
    assert [c.point("bean", k).tp for k in range(5)] == [4, 3, 2, 1, 0]
    assert c.ap("bean") == 1.0
    assert c.best_f1("bean") == (1.0, 0.1)
    assert abs(c.at(0.1)["bean"].avg_acc - 0.02) <= 1e-15 and math.isnan(c.at(0.9)["bean"].avg_acc)
    # no ground truth: NaN, skipped by the mean ('maize' has none either -> the mean itself is NaN)
    c = hand_curve(args, grid, [(0.8, 0)], 0)
    assert math.isnan(c.ap("bean")) and math.isnan(c.mean_ap("anchor"))
    # no detections: precision is 0 by Evaluation's convention (npos > 0), recall 0 -> AP 0; F1 0 everywhere, first threshold wins
    c = hand_curve(args, grid, [], 3)
    assert c.ap("bean") == 0.0 and c.best_f1("bean") == (0.0, 0.1)
    assert c.mean_ap("anchor") == 0.0                                            # 'maize' (NaN) skipped
    # a non-monotone precision: miss, hit, hit, miss, hit over 4 ground truths, scores 0.95 .. 0.15
    #   t     0.9   0.7   0.5   0.3   0.1
    #   tp/nd 0/1   1/2   2/3   2/4   3/5      precision 0, 1/2, 2/3, 1/2, 3/5   recall 0, 1/4, 2/4, 2/4, 3/4
    #   envelope (max over lower thresholds): 2/3, 2/3, 2/3, 3/5, 3/5
    #   AP = 0 * 2/3 + 1/4 * 2/3 + 1/4 * 2/3 + 0 * 3/5 + 1/4 * 3/5
    c = hand_curve(args, grid, [(0.95, 0), (0.75, 1), (0.55, 1), (0.35, 0), (0.15, 1)], 4)
    assert [(c.point("bean", k).tp, c.point("bean", k).ndet) for k in range(5)] == [(3, 5), (2, 4), (2, 3), (1, 2), (0, 1)]
    assert abs(c.ap("bean") - (0.25 * 2 / 3 + 0.25 * 2 / 3 + 0.25 * 0.6)) <= 1e-15
    raw_area = 0.25 * 0.5 + 0.25 * 2 / 3 + 0.25 * 0.6                            # without the envelope: smaller
    assert c.ap("bean") > raw_area
    # F1 = 2 tp / (npos + ndet): 6/9, 4/8, 4/7, 2/6, 0/5 -> the maximum 2/3 at the lowest threshold
    assert c.best_f1("bean") == (6 / 9, 0.1)
    # two equal maxima: the first in ascending order
    c = hand_curve(args, grid, [(0.8, 1), (0.6, 0), (0.4, 1)], 2)                # F1: 4/5 (t .1, .3), 2/4 (.5), 2/3 (.7), 0 (.9)
    assert c.best_f1("bean") == (0.8, 0.1)
    with pytest.raises(KeyError):
        c.at(0.2)


def test_default_grid_and_threshold_handling():
    from structuredetector_amd.model.pr_curve import PrCurve, default_grid
    assert np.array_equal(default_grid(0.5), np.asarray([k / 100 for k in range(1, 100)]))
    g = default_grid(0.055)
    assert len(g) == 100 and (np.diff(g) > 0).all() and 0.055 in g
    c = PrCurve(R.make_args(conf_threshold=0.055))
    assert len(c.thresholds) == 100 and set(c.at(0.055)) == {"bean", "maize", "leaf"}
    assert np.array_equal(PrCurve(R.make_args(), [0.5, 0.1, 0.5]).thresholds, [0.1, 0.5])


def test_merge_of_two_halves_equals_the_whole():
    args = R.make_args(parts=("leaf", "ear"))
    case = R.random_case(np.random.default_rng(77), args, 16, 20, 40, 5, tied=False)
    whole = curve_of(args, case)
    merged = curve_of(args, case, images=slice(0, 8)).merge(curve_of(args, case, images=slice(8, 16)))
    assert merged.images == whole.images == 16
    hits = 0
    for g in ("anchor", "part"):
        for n, t in whole.tables[g].items():
            m = merged.tables[g][n]
            assert np.array_equal(m.tp, t.tp) and np.array_equal(m.ndet, t.ndet) and m.npos == t.npos and m.tp.dtype == np.int64
            # the summation order differs: N * 2^-53 relative for N <= 1e6 hits is below 1e-9
            assert np.allclose(m.acc_sum, t.acc_sum, rtol=1e-9, atol=0)
            hits += int(t.tp[0])
    assert hits > 20


def test_csv_round_trip(tmp_path):
    from structuredetector_amd.model.pr_curve import CSV_HEADER, PrCurve
    args = R.make_args()
    curve = curve_of(args, R.random_case(np.random.default_rng(5), args, 4, 8, 12, 4))
    curve.save_csv(tmp_path / "pr.csv")
    rows = PrCurve.read_csv(tmp_path / "pr.csv")
    assert (tmp_path / "pr.csv").read_text().splitlines()[0] == ",".join(CSV_HEADER)
    assert len(rows) == 3 * 99
    for got, want in zip(rows, curve.rows()):
        assert got[:6] == want[:6]
        for a, b in zip(got[6:], want[6:]):
            assert a == b or (math.isnan(a) and math.isnan(b))                   # bit for bit: floats are written with repr
    assert any(r[3] > 0 for r in rows)
    text = repr(curve)
    assert "mean AP" in text and "best f1" in text and "bean" in text


def test_flags():
    from structuredetector_amd.utils.args import Arguments
    parser = Arguments().parser
    ns = parser.parse_args([])
    assert ns.pr_curve is False and ns.csv_pr_path is None
    ns = parser.parse_args(["--pr_curve", "--save_csv_pr", "curves.csv"])
    assert ns.pr_curve is True and str(ns.csv_pr_path) == "curves.csv"
    text = parser.format_help()
    assert "--pr_curve" in text and "--max_objects" in text and "--save_csv_pr PATH" in text


def test_sd_eval_match_rejects_bad_arguments_without_touching_the_gpu():
    import ctypes as C

    from structuredetector_amd import _lib as L
    lib = L.lib()
    assert "sd_eval_match" in L.declared_symbols()
    INVALID, ALIGN = -1, -3
    d = C.c_double

    def call(a=16, p=32, B=1, K=1, P=1, xy=48, cls=64, off=80, G=1, img=96, match=112, dist=128):
        return lib.sd_eval_match(a, p, B, K, P, xy, cls, off, G, img, d(4.0), d(4.0), match, dist, 0)

    for name in ("a", "p", "xy", "cls", "off", "img", "match", "dist"):
        assert call(**{name: 0}) == INVALID and b"sd_eval_match: null pointer" in lib.sd_last_error(), name
    for kw in (dict(B=0), dict(K=0), dict(P=0), dict(B=-2), dict(K=-1), dict(P=-1)):
        assert call(**kw) == INVALID and b"bad sizes" in lib.sd_last_error(), kw
    assert call(K=1025) == INVALID and b"out of range" in lib.sd_last_error()      # beyond SD_MAX_TOPK, the decoder's own limit
    assert call(P=1025) == INVALID
    assert call(G=-1) == INVALID and b"negative" in lib.sd_last_error()
    assert lib.sd_eval_match(16, 32, 1, 1, 1, 48, 64, 80, 1, 96, d(float("nan")), d(4.0), 112, 128, 0) == INVALID
    for kw in (dict(a=24), dict(p=36), dict(xy=56), dict(cls=66), dict(off=82), dict(img=100), dict(match=114), dict(dist=132)):
        assert call(**kw) == ALIGN and b"misaligned" in lib.sd_last_error(), kw
