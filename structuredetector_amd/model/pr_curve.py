"""`PrCurve`: the anchor-location and part-location metrics of `Evaluator` at EVERY confidence threshold of a grid, from one matching pass
(`evaluate --pr_curve`).  No reference counterpart: the reference reports one operating point, `--conf_threshold`.

The Evaluator's matching is greedy by descending score and a prediction only ever tries its nearest ground truth, so whether top-k slot
i is a hit depends only on the slots ranked above it -- and all of those are present at every threshold that keeps i.  `sd_eval_match`
(csrc/sd_eval.hip) therefore labels every slot of the decoder's packed result a hit or a miss ONCE, on the device; the host bins the
slots by score (`np.searchsorted`) and the counters at threshold t are prefix counts.  The counting rules are the decoder's own and are
asymmetric: an anchor slot counts at t iff score > t (`Decoder._assemble`: `asc > conf_thresh`), a raw part slot iff not score < t.

CSI and the count-classification metric are NOT swept: the part-to-anchor grouping changes non-monotonically when an anchor drops out,
so they are no prefix sums; they stay at the single `--conf_threshold`.  The top-k truncation bounds `ndet` at low thresholds (raise
--max_objects / --max_parts), as `maxDets` does elsewhere.
"""
from __future__ import annotations

import csv
import math

import numpy as np

from .evaluator import Evaluation

GROUPS = ("anchor", "part")
CSV_HEADER = ("group", "label", "threshold", "tp", "ndet", "npos", "precision", "recall", "f1", "mean_acc")


def default_grid(conf_threshold=None):
    """k / 100 for k = 1 .. 99, plus `conf_threshold` when it is not on the grid; sorted, unique."""
    grid = [k / 100 for k in range(1, 100)]
    if conf_threshold is not None:
        grid.append(float(conf_threshold))
    return np.unique(np.asarray(grid, np.float64))


class CurvePoint(Evaluation):
    """One operating point of a curve: an `Evaluation` (tp, npos, ndet and its precision / recall / F1 conventions) whose mean accuracy
    comes from the curve's running sum instead of a list of distances.  The standard error is not kept."""

    def __init__(self, tp, npos, ndet, acc_sum):
        super().__init__(int(tp), int(npos), int(ndet))
        self.acc_sum = float(acc_sum)

    @property
    def avg_acc(self):
        return self.acc_sum / self.tp if self.tp else float("nan")

    @property
    def acc_err(self):
        return float("nan")


class _Table:
    """Counters of one label over the T thresholds of the grid."""

    def __init__(self, T):
        self.tp = np.zeros(T, np.int64)
        self.ndet = np.zeros(T, np.int64)
        self.npos = np.int64(0)
        self.acc_sum = np.zeros(T, np.float64)

    def add(self, other):
        self.tp += other.tp; self.ndet += other.ndet; self.acc_sum += other.acc_sum
        self.npos = np.int64(self.npos + other.npos)


def _suffix_sums(hist):
    """hist (.., T + 1): entry n counts the slots kept by exactly the n lowest thresholds -> (.., T): the slots kept at threshold k."""
    return np.cumsum(hist[..., ::-1], axis=-1)[..., ::-1][..., 1:]


class PrCurve:
    def __init__(self, args, thresholds=None):
        self.args = args
        grid = default_grid(getattr(args, "conf_threshold", None)) if thresholds is None else np.unique(np.asarray(thresholds, np.float64))
        assert grid.ndim == 1 and len(grid) > 0 and np.isfinite(grid).all(), "the threshold grid must be a non-empty list of finite numbers"
        self.thresholds = grid
        self.names = {"anchor": list(args.labels.keys()), "part": list(args.parts.keys())}
        self._class_ids = {"anchor": [args.labels[n] for n in self.names["anchor"]], "part": [args.parts[n] for n in self.names["part"]]}
        self.tables = {g: {n: _Table(len(grid)) for n in self.names[g]} for g in GROUPS}
        self.images = 0
        self.redone = 0                          # batches matched again from a two-launch decode (non-zero decoder status)

    # ------------------------------------------------------------------ accumulation
    def add_records(self, group, score, cls, match, dist, side, gt_cls):
        """Bin one batch of matched slots of one list.  score, cls, match, dist: (B, L) arrays over the slots (fp32 score and class words of
        the packed list, `sd_eval_match`'s match / dist); side: (B,) min(img_size) per image; gt_cls: the classes of the batch's ground
        truths of this group (any shape).  Vectorised: one searchsorted and three bincounts for all labels."""
        thr, T = self.thresholds, len(self.thresholds)
        score = np.asarray(score, np.float64)
        cls = np.asarray(cls).astype(np.int64)
        hit = np.asarray(match) >= 0
        ids = self._class_ids[group]
        C = (max(ids) + 1) if ids else 0
        # anchors: kept iff score > t, i.e. by the thresholds strictly below the score; parts: iff not score < t, i.e. t <= score
        kept = np.searchsorted(thr, score, side="left" if group == "anchor" else "right")
        kept = np.where(np.isnan(score), T if group == "part" else 0, kept)      # `not nan < t` holds for every t, `nan > t` for none
        known = (cls >= 0) & (cls < C)
        idx = np.where(known, cls, 0) * (T + 1) + kept
        ndet = np.bincount(idx[known], minlength=C * (T + 1)).reshape(C, T + 1)
        sel = known & hit
        tp = np.bincount(idx[sel], minlength=C * (T + 1)).reshape(C, T + 1)
        acc = np.asarray(dist, np.float64) / np.asarray(side, np.float64).reshape(-1, 1)
        acc_sum = np.bincount(idx[sel], weights=acc[sel], minlength=C * (T + 1)).reshape(C, T + 1)
        ndet, tp, acc_sum = _suffix_sums(ndet), _suffix_sums(tp), _suffix_sums(acc_sum)
        npos = np.bincount(np.asarray(gt_cls, np.int64).reshape(-1).clip(min=-1) + 1, minlength=C + 1)[1:]
        for name, c in zip(self.names[group], ids):
            t = self.tables[group][name]
            t.tp += tp[c]; t.ndet += ndet[c]; t.acc_sum += acc_sum[c]
            t.npos = np.int64(t.npos + (npos[c] if c < len(npos) else 0))

    def ground_truth_tables(self, annotations):
        """The kernel's ground-truth tables of one batch, from annotations in network-input pixels with `img_size` (what
        `Evaluator.accumulate` receives): (gt_xy (G, 2) float64 in source-image pixels, gt_cls (G,) int32, gt_off (2B + 1,) int32,
        img (B, 3) float64 = fx, fy, thr per image, side (B,) float64)."""
        a = self.args
        B = len(annotations)
        xy, cls, off = [], [], [0]
        img = np.empty((B, 3), np.float64)
        side = np.empty(B, np.float64)
        for b, ann in enumerate(annotations):
            w, h = ann.img_size
            img[b] = (w / a.width, h / a.height, min(w, h) * a.dist_threshold)
            side[b] = min(w, h)
        for b, ann in enumerate(annotations):
            fx, fy = img[b, 0], img[b, 1]
            for o in ann.objects:
                xy.append((o.anchor.x * fx, o.anchor.y * fy)); cls.append(a.labels.get(o.name, -1))
            off.append(len(cls))
        for b, ann in enumerate(annotations):
            fx, fy = img[b, 0], img[b, 1]
            for o in ann.objects:
                for kp in o.parts:
                    xy.append((kp.x * fx, kp.y * fy)); cls.append(a.parts.get(kp.kind, -1))
            off.append(len(cls))
        return (np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(cls, np.int32), np.asarray(off, np.int32), img, side)

    def submit(self, decoder, outputs, annotations, packed=None):
        """Queue the matching of one decoded batch WITHOUT a host wait (mirrors `Decoder.submit`): uploads the ground-truth tables from
        pinned memory, launches `sd_eval_match` on the packed result and starts the copy of match / dist / status into a pinned buffer.
        `packed`: a packed buffer of this batch decoded with the exact top-k (e.g. `PendingDecode.packed` of a `submit(...,
        with_raw_parts=True)`); None: the batch is decoded here.  Returns a `PendingCurve`; `.result()` waits and bins."""
        a = self.args
        states = []
        if packed is None:
            packed, _ = decoder.decode_packed(outputs, a.conf_threshold, a.decoder_dist_thresh, exact_topk=True, state_out=states)
        return PendingCurve(self, decoder, outputs, annotations, packed, states[0] if states else None)

    # ------------------------------------------------------------------ queries
    def _index(self, t):
        k = int(np.searchsorted(self.thresholds, t))
        if k >= len(self.thresholds) or self.thresholds[k] != t:
            raise KeyError(f"PrCurve: {t!r} is not a threshold of the grid")
        return k

    def _table(self, label, group=None):
        for g in GROUPS if group is None else (group,):
            if label in self.tables[g]:
                return self.tables[g][label]
        raise KeyError(f"PrCurve: no label {label!r}")

    def point(self, label, k, group=None):
        t = self._table(label, group)
        return CurvePoint(t.tp[k], t.npos, t.ndet[k], t.acc_sum[k])

    def at(self, t, group=None):
        """{label: CurvePoint} at grid threshold t -- tp / npos / ndet with `Evaluation`'s precision / recall / F1, and the mean accuracy
        as `.avg_acc`.  group: "anchor", "part", or None for both (anchor labels first, like `Evaluator.kps_eval`)."""
        k = self._index(t)
        return {n: self.point(n, k, g) for g in (GROUPS if group is None else (group,)) for n in self.names[g]}

    def ap(self, label, group=None):
        """Area under the right-to-left monotone precision envelope over recall, on the grid's operating points: thresholds from the
        highest down, sum of (R_k - R_{k-1}) * max_{k' >= k} P_k' with R_0 = 0.  NaN when the label has no ground truth."""
        t = self._table(label, group)
        if t.npos == 0:
            return float("nan")
        pts = [self.point(label, k, group) for k in range(len(self.thresholds) - 1, -1, -1)]
        prec = [float(p.precision) for p in pts]
        for k in range(len(prec) - 2, -1, -1):
            prec[k] = max(prec[k], prec[k + 1])
        area, prev = 0.0, 0.0
        for p, env in zip(pts, prec):
            r = float(p.recall)
            area += (r - prev) * env
            prev = r
        return area

    def mean_ap(self, group=None):
        """Mean of `ap` over the labels of the group(s), labels without ground truth (NaN) skipped; NaN when none is left."""
        vals = [self.ap(n, g) for g in (GROUPS if group is None else (group,)) for n in self.names[g]]
        vals = [v for v in vals if not math.isnan(v)]
        return sum(vals) / len(vals) if vals else float("nan")

    def best_f1(self, label, group=None):
        """(F1, threshold) of the best operating point: the FIRST maximum when scanning the thresholds in ascending order."""
        best, where = -1.0, None
        for k, thr in enumerate(self.thresholds):
            f1 = float(self.point(label, k, group).f1_score)
            if f1 > best:
                best, where = f1, float(thr)
        return best, where

    def merge(self, other):
        """Sum the tables of another curve over the same grid and labels (another rank's shard)."""
        assert np.array_equal(self.thresholds, other.thresholds) and self.names == other.names, "PrCurve.merge: different grids or labels"
        for g in GROUPS:
            for n, t in self.tables[g].items():
                t.add(other.tables[g][n])
        self.images += other.images
        self.redone += other.redone
        return self

    # ------------------------------------------------------------------ reporting
    def rows(self):
        """Per group, label and threshold: (group, label, threshold, tp, ndet, npos, precision, recall, F1, mean accuracy)."""
        for g in GROUPS:
            for n in self.names[g]:
                for k, thr in enumerate(self.thresholds):
                    p = self.point(n, k, g)
                    yield (g, n, float(thr), p.tp, p.ndet, p.npos, float(p.precision), float(p.recall), float(p.f1_score), float(p.avg_acc))

    def save_csv(self, path):
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(CSV_HEADER)
            for row in self.rows():
                w.writerow([repr(v) if isinstance(v, float) else v for v in row])      # repr: floats read back to the same bits

    @staticmethod
    def read_csv(path):
        """The rows `save_csv` wrote, typed as `rows()` yields them."""
        with open(path, newline="") as f:
            r = csv.reader(f)
            assert tuple(next(r)) == CSV_HEADER, "not a PrCurve CSV"
            return [(g, n, float(t), int(tp), int(ndet), int(npos), float(p), float(rc), float(f1), float(acc))
                    for g, n, t, tp, ndet, npos, p, rc, f1, acc in r]

    def summary(self):
        """Per group: [(label, AP, best F1, its threshold, CurvePoint at --conf_threshold)], and the group's mean AP."""
        conf = float(self.args.conf_threshold)
        on_grid = conf in self.thresholds
        out = {}
        for g in GROUPS:
            lines = []
            for n in self.names[g]:
                f1, thr = self.best_f1(n, g)
                lines.append((n, self.ap(n, g), f1, thr, self.point(n, self._index(conf), g) if on_grid else None))
            out[g] = (lines, self.mean_ap(g))
        return out

    def __repr__(self):
        text = ""
        for g, (lines, mean) in self.summary().items():
            text += f"PR curve, {g} location ({len(self.thresholds)} thresholds, {self.images} images): mean AP {mean:.2%}\n"
            for n, ap, f1, thr, p in lines:
                at = f", at {self.args.conf_threshold}: prec {p.precision:.2%} rec {p.recall:.2%} f1 {p.f1_score:.2%}" if p is not None else ""
                text += f"  {n}: AP {ap:.2%}, best f1 {f1:.2%} at {thr:g}{at}\n"
        return text

    def pretty_print(self):
        try:
            from rich import print as rprint
            from rich.table import Column, Table
        except ImportError:                                    # plain text when rich is absent
            print(repr(self))
            return
        conf = self.args.conf_threshold
        heads = ("AP", "Best F1", "at thr.", f"Prec. @{conf:g}", f"Rec. @{conf:g}", f"F1 @{conf:g}")
        for g, (lines, mean) in self.summary().items():
            table = Table(Column("Label", style="bold"), *[Column(h, justify="right") for h in heads],
                          title=f"PR curve: {g.capitalize()} Location ({len(self.thresholds)} thresholds)")
            for n, ap, f1, thr, p in lines:
                at = (f"{p.precision:.2%}", f"{p.recall:.2%}", f"{p.f1_score:.2%}") if p is not None else ("-", "-", "-")
                table.add_row(n, f"{ap:.2%}", f"{f1:.2%}", f"{thr:g}", *at)
            if len(lines) > 1:
                table.add_row("Mean", f"{mean:.2%}", "", "", "", "", "", style="bold")
            rprint(table)


class PendingCurve:
    """A matching in flight (`PrCurve.submit`): device tables, the pinned host copies and the event after which they are complete."""

    def __init__(self, curve, decoder, outputs, annotations, packed, state):
        import torch

        from .. import _lib as L
        self.curve, self.decoder, self.outputs, self.packed, self.state = curve, decoder, outputs, packed, state
        dev = packed.device
        self.state_key = (dev.index if dev.index is not None else torch.cuda.current_device(), L.stream())
        B, K, P = len(annotations), decoder.max_objects, decoder.max_parts
        out_h, out_w = outputs["offsets"].shape[-2:]
        in_h, in_w = decoder._input_size(out_h, out_w)
        self.dims, self.scale = (B, K, P), (in_w / out_w, in_h / out_h)
        gt_xy, gt_cls, gt_off, img, self.side = curve.ground_truth_tables(annotations)
        self.gt_cls, self.gt_off = gt_cls, gt_off
        G = len(gt_cls)
        # one pinned table, one upload: fp64 words first (16-byte aligned: gt_xy at word 0), then the int32 tables
        n64 = 2 * max(G, 1) + 3 * B
        n32 = max(G, 1) + 2 * B + 1
        host = decoder._pinned(-(-(n64 + (n32 + 1) // 2) // 1024) * 1024, torch.float64)      # rounded up: few distinct pool sizes
        h64 = host.numpy()
        h32 = h64[n64:].view(np.int32)
        h64[:2 * G] = gt_xy.reshape(-1)
        h64[2 * max(G, 1):n64] = img.reshape(-1)
        h32[:G] = gt_cls
        h32[max(G, 1):n32] = gt_off
        self.tables_host = host
        self.tables = torch.empty(host.numel(), dtype=torch.float64, device=dev)
        self.tables.copy_(host, non_blocking=True)
        self.G, self.n64 = G, n64
        # match / dist of the kernel + the whole packed result (scores, classes, status) in one pinned buffer
        Lr = K + P
        self.result_dev = torch.empty(B * Lr + (B * Lr + 1) // 2, dtype=torch.float64, device=dev)
        self.host = decoder._pinned(self.result_dev.numel() + (packed.numel() + 1) // 2, torch.float64)
        self.done = torch.cuda.Event()
        self._launch(packed)

    def _launch(self, packed):
        import torch

        from .. import _lib as L
        B, K, P = self.dims
        G, n64 = self.G, self.n64
        base = self.tables.data_ptr()
        gt_xy, img = base, base + 8 * 2 * max(G, 1)
        gt_cls = base + 8 * n64
        gt_off = gt_cls + 4 * max(G, 1)
        dist = self.result_dev.data_ptr()
        match = dist + 8 * B * (K + P)
        a_list = packed.data_ptr()
        p_list = a_list + 4 * B * K * 4
        L.check(L.lib().sd_eval_match(a_list, p_list, B, K, P, gt_xy, gt_cls, gt_off, G, img, self.scale[0], self.scale[1], match, dist,
                                      L.stream()), "sd_eval_match")
        n = self.result_dev.numel()
        self.host[:n].copy_(self.result_dev, non_blocking=True)
        self.host[n:].view(torch.int32)[:packed.numel()].copy_(packed, non_blocking=True)
        self.done.record(torch.cuda.current_stream(packed.device))

    def _views(self):
        B, K, P = self.dims
        Lr = K + P
        n = self.result_dev.numel()
        h = self.host.numpy()
        dist = h[:B * Lr].reshape(B, Lr)
        match = h[B * Lr:n].view(np.int32)[:B * Lr].reshape(B, Lr)
        packed = self.decoder.split_packed(h[n:].view(np.int32)[:self.packed.numel()], B, K, P)
        return dist, match, packed

    def result(self, keep_records=False):
        """Wait for the copies, bin the batch into the curve's tables and give the pinned buffers back.  keep_records: leave copies of
        (anchor_out, part_out, match, dist) in `.records` (tests, tools)."""
        import torch
        dec, curve = self.decoder, self.curve
        B, K, P = self.dims
        self.done.synchronize()
        dist, match, packed = self._views()
        failed = bool(packed["status"].any())
        if failed:
            torch.cuda.current_stream(self.packed.device).synchronize()
        if self.state is not None:
            dec._release_state(self.state, self.state_key, failed)
            self.state = None
        if failed:
            # a selector of the one-launch decoder gave up its bounded wait: match again from the two-launch decoder, as PendingDecode does
            curve.redone += 1
            a = curve.args
            self.packed, _ = dec.decode_packed(self.outputs, a.conf_threshold, a.decoder_dist_thresh, exact_topk=True, fused=False)
            self._launch(self.packed)
            self.done.synchronize()
            dist, match, packed = self._views()
            if packed["status"].any():
                from .. import _lib as L
                raise L.SdError(f"sd_decode: non-zero status for image(s) {np.nonzero(packed['status'])[0].tolist()}")
        a_out, p_out = packed["anchor_out"], packed["part_out"]
        off = self.gt_off
        curve.add_records("anchor", a_out[..., 2], a_out[..., 3], match[:, :K], dist[:, :K], self.side, self.gt_cls[off[0]:off[B]])
        curve.add_records("part", p_out[..., 2], p_out[..., 3], match[:, K:], dist[:, K:], self.side, self.gt_cls[off[B]:off[2 * B]])
        curve.images += B
        self.records = (a_out.copy(), p_out.copy(), match.copy(), dist.copy()) if keep_records else None
        pool = dec._host_pool
        pool[(self.host.numel(), self.host.dtype)].append(self.host)
        pool[(self.tables_host.numel(), self.tables_host.dtype)].append(self.tables_host)
        self.outputs = self.packed = self.host = self.tables_host = self.tables = self.result_dev = None
        return curve
