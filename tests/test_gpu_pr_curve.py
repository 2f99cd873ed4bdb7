"""`evaluate --pr_curve` on the GPU: `sd_eval_match` against the numpy reference (tests/pr_curve_ref.py) over its shapes and exact
hand-made cases, `PrCurve` against decoder + Evaluator at single thresholds for the three decoders, and the CLI (directory, --tta,
--synthetic, two ranks over gloo)."""
import json
import os
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch

from tests import pr_curve_ref as R

pytestmark = pytest.mark.gpu

CHUNK = 1024                                                     # SD_EVAL_GT_CHUNK (include/sdnet_hip.h)


# --------------------------------------------------------------------------------------------- the kernel
def run_kernel(case):
    from structuredetector_amd import _lib as L
    dev = torch.device("cuda")
    a, p = torch.from_numpy(case["a_list"]).to(dev), torch.from_numpy(case["p_list"]).to(dev)
    B, K, P = a.shape[0], a.shape[1], p.shape[1]
    G = len(case["gt_cls"])
    xy = torch.from_numpy(case["gt_xy"] if G else np.zeros((1, 2))).to(dev)
    cls = torch.from_numpy(case["gt_cls"] if G else np.zeros(1, np.int32)).to(dev)
    off, img = torch.from_numpy(case["gt_off"]).to(dev), torch.from_numpy(case["img"]).to(dev)
    match = torch.full((B, K + P), -7, dtype=torch.int32, device=dev)
    dist = torch.full((B, K + P), float("nan"), dtype=torch.float64, device=dev)
    L.check(L.lib().sd_eval_match(a.data_ptr(), p.data_ptr(), B, K, P, xy.data_ptr(), cls.data_ptr(), off.data_ptr(), G, img.data_ptr(),
                                  case["sx"], case["sy"], match.data_ptr(), dist.data_ptr(), L.stream()), "sd_eval_match")
    return match.cpu().numpy(), dist.cpu().numpy()


def assert_matches_reference(case, what):
    want_m, want_d = R.match_ref(case)
    got_m, got_d = run_kernel(case)
    assert np.array_equal(got_m, want_m), (what, np.argwhere(got_m != want_m)[:5].tolist())
    inf = np.isinf(want_d)
    assert np.array_equal(np.isinf(got_d), inf), what
    # two hypot implementations, each correct to below 1 ulp, can differ by 2
    assert (np.abs(got_d[~inf] - want_d[~inf]) <= 4 * np.spacing(want_d[~inf])).all(), what
    return want_m, want_d


def big_segment_case(args):
    """One anchor segment of CHUNK + 1 ground truths on a 40 x 26 lattice; the slots sit near lattice points of both chunks, two of them
    (slots 1 and 4) nearest to the LAST ground truth: the claim is settled in the second chunk's pass."""
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    rng = np.random.default_rng(9)
    n = CHUNK + 1
    gx, gy = (np.arange(n) % 40) * 3.0 + 1.5, (np.arange(n) // 40) * 4.5 + 1.25
    gx, gy = gx + rng.uniform(-0.2, 0.2, n), gy + rng.uniform(-0.2, 0.2, n)
    objs = [Object("bean", Keypoint("stem", x, y), [Keypoint("leaf", 5.0, 5.0)] if i == 0 else []) for i, (x, y) in enumerate(zip(gx, gy))]
    ann = ImageAnnotation("big.png", objs, (256, 256))
    case = dict(annotations=[ann], sx=4.0, sy=4.0, side=np.asarray([256.0]))
    case["gt_xy"], case["gt_cls"], case["gt_off"], case["img"] = R.gt_tables(args, [ann])
    a = np.zeros((1, 5, 4), np.float32)
    for i, j in enumerate((3, n - 1, 700, CHUNK - 1, n - 1)):
        a[0, i] = ((gx[j] + rng.uniform(-0.5, 0.5)) / 4.0, (gy[j] + rng.uniform(-0.5, 0.5)) / 4.0, 0.9 - 0.1 * i, 0)
    p = np.zeros((1, 7, 6), np.float32)
    p[0, :, :2] = rng.uniform(0, 32, (7, 2))
    p[0, :, 2] = np.linspace(0.9, 0.1, 7)
    case["a_list"], case["p_list"] = a, p
    return case


@pytest.fixture(scope="module")
def kernel_cases():
    """Every random case once, checked on the CPU for the condition under which two correct implementations must agree."""
    args = R.make_args(labels=("bean", "maize", "rye"), parts=("leaf", "ear"), width=128, height=128)
    rng = np.random.default_rng(20261019)
    cases = {
        "one": R.random_case(rng, args, 1, 1, 1, 1, hit_rate=1.0),
        "no_gt": R.random_case(rng, args, 3, 5, 7, 0),
        "empty_class": R.random_case(rng, args, 2, 12, 9, 4, empty_class=1),
        "small": R.random_case(rng, args, 2, 20, 40, 9),
        "stress": R.random_case(rng, args, 2, 512, 512, 300, size=(256, 256), img_sizes=((2048, 1536), (1200, 1600))),
        "chunk_plus_one": big_segment_case(args),
        "b65": R.random_case(rng, args, 65, 3, 4, 2),
    }
    one = cases["one"]                                           # the one slot of each list half a pixel from its one ground truth
    for lst, seg in ((one["a_list"], 0), (one["p_list"], 1)):
        gx, gy = one["gt_xy"][seg] / one["img"][0, :2]
        lst[0, 0, :2] = ((gx + 0.5) / one["sx"], (gy - 0.25) / one["sy"])
        lst[0, 0, 3] = one["gt_cls"][seg]
    # claims on one ground truth from different waves: slots 3 and 300 of image 0's anchor list next to ground truth 17's position
    s = cases["stress"]
    fx, fy = s["img"][0, 0], s["img"][0, 1]
    gx, gy = s["gt_xy"][17] / (fx, fy)
    for i, (dx, dy) in ((3, (0.9, -0.4)), (300, (-0.3, 0.5))):
        s["a_list"][0, i, :2] = ((gx + dx) / s["sx"], (gy + dy) / s["sy"])
        s["a_list"][0, i, 3] = s["gt_cls"][17]
    for name, case in cases.items():
        assert R.well_conditioned(case) is None, (name, R.well_conditioned(case))
    return args, cases


@pytest.mark.parametrize("name", ["one", "no_gt", "empty_class", "small", "stress", "chunk_plus_one", "b65"])
def test_kernel_against_numpy_reference(kernel_cases, name):
    _, cases = kernel_cases
    case = cases[name]
    m, d = assert_matches_reference(case, name)
    K = case["a_list"].shape[1]
    if name == "one":
        assert m.tolist() == [[0, 0]]
    if name == "no_gt":
        assert (m == -1).all() and np.isinf(d).all()
    if name == "empty_class":
        none = case["a_list"][..., 3] == 1
        assert none.any() and np.isinf(d[:, :K][none]).all() and (m[:, :K][none] == -1).all() and (m >= 0).any()
    if name == "small":
        assert (m >= 0).sum() >= 10 and ((m < 0) & np.isfinite(d)).sum() >= 10
    if name == "stress":
        assert m[0, 3] == 17 and m[0, 300] == -1 and d[0, 300] < case["img"][0, 2]          # the later wave's claim loses
        assert (m >= 0).sum() > 300
    if name == "chunk_plus_one":
        assert m[0, :5].tolist() == [3, CHUNK, 700, CHUNK - 1, -1] and d[0, 4] < case["img"][0, 2]
    if name == "b65":
        assert (m[64] >= 0).any() and len(m) == 65


def hand_case(preds, gts, thr):
    """Anchors of one class on integer coordinates (hypot is exact), sx = sy = fx = fy = 1; one part slot without ground truth."""
    a = np.zeros((1, len(preds), 4), np.float32)
    a[0, :, :2] = preds
    a[0, :, 2] = np.linspace(0.9, 0.5, len(preds))
    return dict(a_list=a, p_list=np.zeros((1, 1, 6), np.float32), sx=1.0, sy=1.0, gt_xy=np.asarray(gts, np.float64),
                gt_cls=np.zeros(len(gts), np.int32), gt_off=np.asarray([0, len(gts), len(gts)], np.int32), img=np.asarray([[1.0, 1.0, thr]]))


def test_kernel_exact_hand_made_cases():
    # equal distances: the lower ground-truth index wins
    m, d = run_kernel(hand_case([(5, 5)], [(2, 5), (8, 5)], 4.0))
    assert m[0].tolist() == [0, -1] and d[0, 0] == 3.0 and np.isinf(d[0, 1])
    m, d = run_kernel(hand_case([(5, 5)], [(8, 5), (2, 5)], 4.0))
    assert m[0, 0] == 0 and d[0, 0] == 3.0
    # d == thr: a miss (strict compare); just inside: a hit
    m, d = run_kernel(hand_case([(5, 5)], [(2, 5)], 3.0))
    assert m[0, 0] == -1 and d[0, 0] == 3.0
    m, d = run_kernel(hand_case([(5, 5)], [(2, 5)], np.nextafter(3.0, 4.0)))
    assert m[0, 0] == 0 and d[0, 0] == 3.0
    # two slots nearest to ground truth 0; ground truth 1 lies within the radius of the loser: no second choice
    case = hand_case([(1, 0), (2, 0)], [(0, 0), (5, 0)], 4.0)
    m, d = run_kernel(case)
    assert m[0, :2].tolist() == [0, -1] and d[0, :2].tolist() == [1.0, 2.0]
    assert np.array_equal(m, R.match_ref(case)[0])
    # 3-4-5 triangles, scaled coordinates: X = (x * sx) * fx
    case = hand_case([(3, 4)], [(0, 0), (60, 0)], 60.0)
    case["sx"], case["sy"], case["img"] = 2.0, 2.0, np.asarray([[3.0, 3.0, 60.0]])
    m, d = run_kernel(case)
    assert m[0, 0] == 0 and d[0, 0] == 30.0


# --------------------------------------------------------------------------------------------- decoder level
LOGITS = [3.0, 1.4, 0.4, -0.4, -0.62, -1.4, -2.6]               # sigmoid: 0.953, 0.802, 0.599, 0.401, 0.350, 0.198, 0.069


def planted_head(B, M, N, h, w, seed):
    """Random low logits (sigmoid about 0.01) with planted peaks on a 6-cell lattice; image 0 has an anchor and a part peak of the SAME
    logit (-0.4), so one fp32 score sits in both lists."""
    g = torch.Generator().manual_seed(seed)
    head = torch.randn(B, M + N + 4, h, w, generator=g) * 0.4 - 4.8
    head[:, M + N:M + N + 2] = torch.rand(B, 2, h, w, generator=g)
    head[:, M + N + 2:] = torch.randn(B, 2, h, w, generator=g)
    rng = np.random.default_rng(seed)
    sites = [(3 + 6 * j, 3 + 6 * i) for j in range(h // 6) for i in range(w // 6)]
    for b in range(B):
        order = rng.permutation(len(sites))
        for k in range(5):                                       # anchors: logits 0 .. 4
            y, x = sites[order[k]]
            head[b, int(rng.integers(M)), y, x] = LOGITS[k]
        for k in range(7):
            y, x = sites[order[5 + k]]
            head[b, M + int(rng.integers(N)), y, x] = LOGITS[k]
    return head


def decoder_setup(kind):
    from structuredetector_amd.data import Decoder, FusedOutputDecoder, RawDecoder
    from structuredetector_amd.data.decoders import TiledOutputDecoder
    from structuredetector_amd.utils import ImageAnnotation, Keypoint, Object
    M, N = 2, 3
    args = R.make_args(parts=("leaf", "ear", "tassel"), max_objects=8, max_parts=16)
    h, w = (32, 56) if kind == "tiled" else (32, 32)             # 2 x 1 tiles of 32 x 32 cells that share 8 columns
    head = planted_head(3, M, N, h, w, seed=11).cuda()
    if kind == "logits":
        dec, src = Decoder(args), head
    else:
        dec = FusedOutputDecoder(args) if kind == "fused" else TiledOutputDecoder(args, (2, 1), 8)
        src = RawDecoder(M + N)(head)                            # suppressed probabilities + the regression channels
    out = {"anchor_hm": src[:, :M], "part_hm": src[:, M:M + N], "offsets": src[:, M + N:M + N + 2], "embeddings": src[:, M + N + 2:]}
    # a first decode: ground truths are placed relative to the decoded positions -- near every even slot of the top six (a hit), 12 pixels
    # away from every odd one (a false positive and a false negative)
    packed, (B, K, P, _, _) = dec.decode_packed(out, 0.5, 0.1, exact_topk=True, fused=False)
    first = dec.split_packed(packed.cpu().numpy(), B, K, P)
    in_h, in_w = dec._input_size(h, w)
    assert (in_h, in_w) == (128, 128)
    sx, sy = in_w / w, in_h / h
    rng = np.random.default_rng(5)
    sizes = [(300, 200), (160, 240), (200, 150)]                 # fx != fy != 1
    anns = []
    for b in range(B):
        def points(lst):
            pts = []
            for i in range(6):
                x, y, _, c = lst[b, i].tolist()[:4]
                dx, dy = rng.uniform(-1.5, 1.5, 2) if i % 2 == 0 else rng.choice([-12.0, 12.0], 2)
                pts.append((x * sx + dx, y * sy + dy, int(c)))
            return pts
        anchors, parts = points(first["anchor_out"]), points(first["part_out"])
        objs = [Object(args._r_labels[c], Keypoint("stem", x, y), [Keypoint(args._r_parts[parts[i][2]], parts[i][0], parts[i][1])])
                for i, (x, y, c) in enumerate(anchors)]
        anns.append(ImageAnnotation(f"img_{b}.png", objs, sizes[b]))
    return args, dec, out, anns, first


@pytest.mark.parametrize("kind", ["logits", "fused", "tiled"])
def test_curve_equals_decoder_plus_evaluator_at_single_thresholds(kind):
    from structuredetector_amd.model import Evaluator
    from structuredetector_amd.model.pr_curve import PrCurve
    args, dec, out, anns, first = decoder_setup(kind)
    # an fp32 score present in BOTH lists of image 0 (the planted logit -0.4)
    shared = [s for s in set(first["anchor_out"][0, :, 2].tolist()) & set(first["part_out"][0, :, 2].tolist()) if 0.39 < s < 0.41]
    assert len(shared) == 1, shared
    t_exact = shared[0]
    below, above = float(np.nextafter(t_exact, 0.0)), float(np.nextafter(t_exact, 1.0))
    curve = PrCurve(args, [0.05, 0.3, 0.5, 0.9, t_exact, below, above])
    pending = curve.submit(dec, out, anns)
    assert pending.result(keep_records=True) is curve and curve.images == 3 and curve.redone == 0
    # the records are the reference's on the decoder's own lists
    a_out, p_out, match, dist = pending.records
    case = dict(a_list=a_out, p_list=p_out, sx=pending.scale[0], sy=pending.scale[1])
    case["gt_xy"], case["gt_cls"], case["gt_off"], case["img"] = R.gt_tables(args, anns)
    assert R.well_conditioned(case) is None
    want_m, want_d = R.match_ref(case)
    assert np.array_equal(match, want_m) and np.allclose(dist, want_d, rtol=1e-15, atol=0)
    for t in (0.05, 0.3, 0.5, 0.9, t_exact):
        data = dec(out, conf_thresh=t, return_metadata=True, metadata_fields=("annotation", "raw_parts"))
        ev = Evaluator(args)
        for pred, ann, raw in zip(data["annotation"], anns, data["raw_parts"]):
            ev.accumulate(pred, ann, raw, False, False)
        got = curve.at(t)
        for label, e in list(ev.anchor_eval.items()) + list(ev.part_eval.items()):
            c = got[label]
            assert (c.tp, c.npos, c.ndet) == (e.tp, e.npos, e.ndet), (kind, t, label, (c.tp, c.npos, c.ndet), (e.tp, e.npos, e.ndet))
            if e.tp:
                assert abs(c.avg_acc - e.avg_acc) <= 1e-9, (kind, t, label)
            else:
                assert np.isnan(c.avg_acc)
        if t == 0.3:
            assert any(e.tp > 0 and e.fp > 0 for _, e in ev.anchor_eval.items()) and any(e.tp > 0 and e.fp > 0 for _, e in ev.part_eval.items())
            assert ev.anchor_eval.reduce().fn > 0
    # `>` against `>=`: at the exact score the anchor is out and the part is in
    ndet = lambda t, g: sum(p.ndet for p in curve.at(t, g).values())
    assert ndet(below, "anchor") - ndet(t_exact, "anchor") >= 1 and ndet(t_exact, "anchor") == ndet(above, "anchor")
    assert ndet(below, "part") == ndet(t_exact, "part") and ndet(t_exact, "part") - ndet(above, "part") >= 1
    # a second submission reuses a handed-in packed buffer and doubles every table
    handle = dec.submit(out, with_raw_parts=True)
    again = PrCurve(args, curve.thresholds)
    pend = again.submit(dec, out, anns, packed=handle.packed)
    handle.result()
    pend.result()
    for g in ("anchor", "part"):
        for n, tb in again.tables[g].items():
            ref = curve.tables[g][n]
            assert np.array_equal(tb.tp, ref.tp) and np.array_equal(tb.ndet, ref.ndet) and tb.npos == ref.npos and np.array_equal(tb.acc_sum, ref.acc_sum)


# --------------------------------------------------------------------------------------------- CLI
def counters(evals):
    return {label: (e.tp, e.npos, e.ndet) for label, e in evals.items()}


def evaluator_state(ev):
    return {sec: [(label, e.tp, e.npos, e.ndet, list(e.acc)) for label, e in evals.items()]
            for sec, evals in (("anchor", ev.anchor_eval), ("part", ev.part_eval), ("csi", ev.csi_eval), ("classif", ev.classification_eval))}


def planted_network(heads):
    class PlantedNetwork(torch.nn.Module):
        def __init__(self, args, *a, **kw):
            super().__init__()
            self.dummy = torch.nn.Parameter(torch.zeros(1))
            self.seen = 0

        def forward(self, x):
            h = torch.from_numpy(np.stack(heads[self.seen:self.seen + x.shape[0]])).to(x.device)
            self.seen += x.shape[0]
            return {"anchor_hm": h[:, :2], "part_hm": h[:, 2:3], "offsets": h[:, 3:5], "embeddings": h[:, 5:7]}
    return PlantedNetwork


def same_rows(a, b):
    """CSV rows against `PrCurve.rows()`: equal values, NaN (the mean accuracy of an operating point without hits) equal to NaN."""
    a, b = list(a), list(b)
    return len(a) == len(b) and all(len(ra) == len(rb) and all(x == y or (x != x and y != y) for x, y in zip(ra, rb)) for ra, rb in zip(a, b))


def curve_tables(curve):
    return {g: {n: (t.tp.tolist(), t.ndet.tolist(), int(t.npos), t.acc_sum.tolist()) for n, t in curve.tables[g].items()} for g in ("anchor", "part")}


def test_evaluate_cli_pr_curve_on_16_samples(golden_dir, tmp_path, monkeypatch, capsys):
    from structuredetector_amd.cli import evaluate
    from tests.helpers import write_evaluate16_dir
    g = np.load(golden_dir / "evaluate16.npz")
    heads = write_evaluate16_dir(g, tmp_path / "valid")
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    argv = ["--valid_dir", str(tmp_path / "valid"), "-s", "stem", "--labels", str(tmp_path / "labels.json"), "--eval_batch", "5"]
    monkeypatch.setattr(evaluate, "Network", planted_network(heads))
    plain = evaluate.main(argv)
    assert not hasattr(plain, "pr_curve")
    capsys.readouterr()
    ev = evaluate.main(argv + ["--pr_curve", "--save_csv_pr", str(tmp_path / "pr.csv")])
    text = capsys.readouterr().out
    assert "CSI" in text and "PR curve" in text and "Anchor Location" in text
    assert evaluator_state(ev) == evaluator_state(plain)
    curve = ev.pr_curve
    assert curve.images == 16 and len(curve.thresholds) == 99
    at = curve.at(0.5)
    assert {k: (v.tp, v.npos, v.ndet) for k, v in curve.at(0.5, "anchor").items()} == counters(plain.anchor_eval)
    assert {k: (v.tp, v.npos, v.ndet) for k, v in curve.at(0.5, "part").items()} == counters(plain.part_eval)
    for label, e in list(plain.anchor_eval.items()) + list(plain.part_eval.items()):
        assert e.tp > 0 and abs(at[label].avg_acc - e.avg_acc) <= 1e-9
    for t in ("0.1", "0.7"):
        other = evaluate.main(argv + ["-t", t])
        assert {k: (v.tp, v.npos, v.ndet) for k, v in curve.at(float(t), "anchor").items()} == counters(other.anchor_eval), t
        assert {k: (v.tp, v.npos, v.ndet) for k, v in curve.at(float(t), "part").items()} == counters(other.part_eval), t
    rows = curve.read_csv(tmp_path / "pr.csv")
    assert len(rows) == 3 * 99 and same_rows(rows, curve.rows())
    assert 0 < curve.ap("bean") <= 1 and 0 < curve.mean_ap() <= 1


@pytest.fixture()
def cli_setup(tmp_path, monkeypatch):
    from argparse import Namespace

    from structuredetector_amd.model import Network
    monkeypatch.chdir(tmp_path)
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    torch.manual_seed(3)
    Network(Namespace(labels={"bean": 0, "maize": 1}, parts={"leaf": 0}, fpn_depth=128), pretrained=False).save(tmp_path / "w.pth")
    return tmp_path, ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "-o", str(tmp_path / "w.pth"), "-t", "0.05"]


@pytest.mark.parametrize("tta", [[], ["--tta", "hflip"]], ids=["plain", "hflip"])
def test_evaluate_cli_pr_curve_synthetic(cli_setup, tta):
    """--synthetic 8 (a random network is not confident: -t 0.05), plain and behind the flip TTA: the curve at the threshold equals the
    Evaluator's own counters of the same run, and the CSV is written."""
    from structuredetector_amd.cli import evaluate
    tmp, common = cli_setup
    ev = evaluate.main(common + ["--synthetic", "8", "--pr_curve", "--save_csv_pr", str(tmp / "pr.csv")] + tta)
    curve = ev.pr_curve
    assert curve.images == 8
    assert {k: (v.tp, v.npos, v.ndet) for k, v in curve.at(0.05, "anchor").items()} == counters(ev.anchor_eval)
    assert {k: (v.tp, v.npos, v.ndet) for k, v in curve.at(0.05, "part").items()} == counters(ev.part_eval)
    assert ev.anchor_eval.reduce().npos > 0 and ev.anchor_eval.reduce().ndet > 0
    assert same_rows(curve.read_csv(tmp / "pr.csv"), curve.rows())


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, tmp, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=300))
    try:
        from pathlib import Path

        from structuredetector_amd.cli import evaluate
        from structuredetector_amd.utils.distributed import shard_range
        tmp = Path(tmp)
        heads = np.load(tmp / "heads.npy")
        lo, hi = shard_range(16, rank, world)
        evaluate.Network = planted_network(list(heads[lo:hi]))
        ev = evaluate.main(["--valid_dir", str(tmp / "valid"), "-s", "stem", "--labels", str(tmp / "labels.json"), "--eval_batch", "5",
                            "--pr_curve", "--save_csv_pr", str(tmp / f"pr_w{world}.csv")])
        out[rank] = (curve_tables(ev.pr_curve), ev.pr_curve.images)
    finally:
        dist.destroy_process_group()


def test_evaluate_cli_pr_curve_two_ranks(golden_dir, tmp_path, monkeypatch):
    """Two ranks over gloo on the one GPU give the one-process tables on both ranks: ints exactly, acc_sum to 1e-9 (the shards are summed
    separately); rank 0 alone writes the CSV."""
    import torch.multiprocessing as mp

    from structuredetector_amd.cli import evaluate
    from tests.helpers import write_evaluate16_dir
    g = np.load(golden_dir / "evaluate16.npz")
    heads = write_evaluate16_dir(g, tmp_path / "valid")
    np.save(tmp_path / "heads.npy", np.stack(heads))
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    out = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path), out), nprocs=2, join=True)
    monkeypatch.setattr(evaluate, "Network", planted_network(heads))
    one = evaluate.main(["--valid_dir", str(tmp_path / "valid"), "-s", "stem", "--labels", str(tmp_path / "labels.json"), "--eval_batch", "5",
                         "--pr_curve"])
    want = curve_tables(one.pr_curve)
    for r in range(2):
        got, images = out[r]
        assert images == 16
        for grp in ("anchor", "part"):
            for n, (tp, ndet, npos, acc) in want[grp].items():
                gtp, gndet, gnpos, gacc = got[grp][n]
                assert (gtp, gndet, gnpos) == (tp, ndet, npos), (r, grp, n)
                assert np.allclose(gacc, acc, rtol=1e-9, atol=0), (r, grp, n)
    assert sum(want["anchor"]["bean"][0]) > 0
    assert (tmp_path / "pr_w2.csv").exists()
