"""`LabelNms` (`--label_nms R`) around the bare network and around every test-time wrapper, on a stub net in every form a forward's
output can take; what it is for (a planted duplicate decodes to one object); and the seams of `evaluate`, `detect` and `Predictor`."""
import json

import numpy as np
import pytest
import torch

from tests.label_nms_ref import expected_label_nms, expected_nms5_labels
from tests.test_gpu_tta import ann_key, default_label_args
from tests.test_gpu_view_wrappers import B, StubNet, images_at

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("H,W", [(32, 32), (32, 64)])
def test_label_nms_around_the_bare_net_equals_the_composition(H, W, R):
    """One raw head tensor, its four channel-slice views (ONE `sd_nms5` launch over the M + N channels), or four tensors of their own (one
    launch on the anchors, one on the parts), then `sd_label_nms` on the anchor maps: the same maps, the head's own regressions."""
    from structuredetector_amd.data.decoders import TtaOutput
    from structuredetector_amd.model.label_nms import LabelNms
    from structuredetector_amd.utils.ops import clamped_sigmoid, nms
    args = default_label_args(width=W, height=H)
    M, N = len(args.labels), len(args.parts)
    x = images_at((W, H))
    for config in ("a", "b", "c"):
        net = StubNet(args, config)
        got = LabelNms(net, args, R)(x)
        head = net.heads[0]
        want = expected_nms5_labels(head[:, :M + N], M, R)
        assert isinstance(got, TtaOutput) and set(got) == {"anchor_hm", "part_hm", "offsets", "embeddings"}
        assert same_bits(got["anchor_hm"], want[:, :M]) and same_bits(got["part_hm"], want[:, M:]), config
        assert torch.equal(got["offsets"], head[:, M + N:M + N + 2]) and torch.equal(got["embeddings"], head[:, M + N + 2:]), config
        if config != "c":
            for k in ("offsets", "embeddings"):
                assert got[k].untyped_storage().data_ptr() == head.untyped_storage().data_ptr(), (config, k)
        assert 0 < int((got["anchor_hm"] > 0).sum()) < int((nms(clamped_sigmoid(head[:, :M])) > 0).sum())


class Recorder:
    """`inner` with its last output kept."""

    def __init__(self, inner):
        self.inner, self.needs_sources, self.out = inner, getattr(inner, "needs_sources", False), None

    def __call__(self, images, at_size=None):
        self.out = self.inner(images, at_size=at_size) if self.needs_sources else self.inner(images)
        return self.out


def wrappers(net, args):
    from structuredetector_amd.model.tiles import TiledNet
    from structuredetector_amd.model.tta import FlipTta, ScaleTta, TransposeTta
    return {"flip": FlipTta(net, args, "hvflip"), "scales": ScaleTta(net, args, [(32, 32), (64, 64)], "hflip"),
            "transpose": TransposeTta(net, args, "hflip"), "tiles": TiledNet(net, args, (2, 1), 0)}


@pytest.mark.parametrize("config", ["a", "b", "c"])
@pytest.mark.parametrize("name", ["flip", "scales", "transpose", "tiles"])
def test_label_nms_around_each_wrapper_replaces_the_anchor_maps_only(name, config):
    from structuredetector_amd.data.decoders import TtaOutput
    from structuredetector_amd.model.label_nms import LabelNms, label_nms
    R = 2
    args = default_label_args(width=32, height=32)
    inner = Recorder(wrappers(StubNet(args, config), args)[name])
    net = LabelNms(inner, args, R)
    assert net.needs_sources == (name in ("scales", "tiles"))
    got = net(images_at((32, 32)), at_size=images_at) if net.needs_sources else net(images_at((32, 32)))
    assert isinstance(got, TtaOutput) and isinstance(inner.out, TtaOutput)
    for k in ("part_hm", "offsets", "embeddings"):
        assert got[k] is inner.out[k], k
    anchors = inner.out["anchor_hm"]
    assert same_bits(got["anchor_hm"], label_nms(anchors, R)) and same_bits(got["anchor_hm"], expected_label_nms(anchors, R))
    assert 0 < int((got["anchor_hm"] > 0).sum()) < int((anchors > 0).sum())


def test_a_planted_duplicate_decodes_to_one_object_with_all_its_parts():
    """The same object under two labels one cell apart, a part on either side, each pointing at the nearer peak: two objects with one
    part each without the flag, ONE object (the stronger label) with both parts with it."""
    from structuredetector_amd.data import Decoder
    from structuredetector_amd.model.label_nms import LabelNms
    from structuredetector_amd.model.tta import tta_decoder
    from tests.test_host_cpu import make_args
    dev = torch.device("cuda")
    M, N, h, w = 2, 1, 32, 32
    args = make_args(M, N, 20, 40, device=dev, conf_threshold=0.5)
    logit = lambda p: float(np.log(p / (1 - p)))
    ax, ay = 10, 12
    head = torch.zeros(1, M + N + 4, h, w, device=dev)
    head[:, :M + N] = -8.0
    head[0, 1, ay, ax] = logit(0.9)
    head[0, 0, ay, ax + 1] = logit(0.8)
    parts = [(ax - 3, ay, ax), (ax + 4, ay + 1, ax + 1)]                   # (px, py, the anchor column its embedding points at)
    for px, py, tx in parts:
        head[0, M, py, px] = logit(0.7)
        head[0, M + N + 2, py, px], head[0, M + N + 3, py, px] = float(tx - px), float(ay - py)

    def planted(x):
        return {"anchor_hm": head[:, :M], "part_hm": head[:, M:M + N], "offsets": head[:, M + N:M + N + 2], "embeddings": head[:, M + N + 2:]}

    x = torch.zeros(1, 3, 4 * h, 4 * w, device=dev)
    plain = Decoder(args)(planted(x))[0]
    assert sorted((o.name, o.x, o.y, [(p.x, p.y) for p in o.parts]) for o in plain.objects) == [
        ("label0", 4.0 * (ax + 1), 4.0 * ay, [(4.0 * (ax + 4), 4.0 * (ay + 1))]), ("label1", 4.0 * ax, 4.0 * ay, [(4.0 * (ax - 3), 4.0 * ay)])]
    got = tta_decoder(args)(LabelNms(planted, args, 1)(x))[0]
    assert len(got.objects) == 1
    obj = got.objects[0]
    assert (obj.name, obj.x, obj.y) == ("label1", 4.0 * ax, 4.0 * ay) and abs(obj.anchor.score - 0.9) <= 1e-6
    assert sorted((p.x, p.y) for p in obj.parts) == sorted((4.0 * px, 4.0 * py) for px, py, _ in parts)


def evaluator_state(ev):
    return {sec: [(label, e.tp, e.npos, e.ndet, list(e.acc)) for label, e in evals.items()]
            for sec, evals in (("anchor", ev.anchor_eval), ("part", ev.part_eval), ("csi", ev.csi_eval), ("classif", ev.classification_eval))}


def curve_tables(curve):
    return {g: {n: (t.tp.tolist(), t.ndet.tolist(), int(t.npos), t.acc_sum.tolist()) for n, t in curve.tables[g].items()} for g in ("anchor", "part")}


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_evaluate_with_one_label_within_the_5x5_window_changes_nothing(golden_dir, tmp_path, monkeypatch, capsys, bf16):
    """One label and R = 2 is the identity on the maps: `evaluate --label_nms 2` on the 16-sample directory (every object relabelled to the
    one label) returns the plain run's evaluator state and `--pr_curve` tables, although the maps take the other decoder."""
    from argparse import Namespace
    from structuredetector_amd.cli import evaluate
    from structuredetector_amd.model import Network
    from tests.helpers import write_evaluate16_dir
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "valid")
    for path in sorted((tmp_path / "valid").glob("*.json")):
        js = json.loads(path.read_text())
        for o in js["objects"]:
            o["label"] = "bean"
        path.write_text(json.dumps(js))
    monkeypatch.chdir(tmp_path)
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean"], "parts": ["leaf"]}))
    torch.manual_seed(3)
    Network(Namespace(labels={"bean": 0}, parts={"leaf": 0}, fpn_depth=128), pretrained=False).save(tmp_path / "w.pth")
    argv = ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "-o", str(tmp_path / "w.pth"), "-t", "0.05",
            "--valid_dir", str(tmp_path / "valid"), "--eval_batch", "5", "--pr_curve"] + (["--bf16_inference"] if bf16 else [])
    plain = evaluate.main(argv)
    assert "label_nms" not in capsys.readouterr().out
    flagged = evaluate.main(argv + ["--label_nms", "2"])
    assert "label_nms: anchor peaks are suppressed across the 1 label maps within 2 cells" in capsys.readouterr().out
    assert evaluator_state(flagged) == evaluator_state(plain)
    assert curve_tables(flagged.pr_curve) == curve_tables(plain.pr_curve) and flagged.pr_curve.images == 16
    assert plain.anchor_eval.reduce().npos > 0 and plain.anchor_eval.reduce().ndet > 0


@pytest.fixture()
def cli_setup(tmp_path, monkeypatch):
    from argparse import Namespace
    from structuredetector_amd.model import Network
    monkeypatch.chdir(tmp_path)
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    torch.manual_seed(3)
    Network(Namespace(labels={"bean": 0, "maize": 1}, parts={"leaf": 0}, fpn_depth=128), pretrained=False).save(tmp_path / "w.pth")
    return tmp_path, ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "-o", str(tmp_path / "w.pth"), "-t", "0.05"]


def test_predictor_with_label_nms(cli_setup):
    from PIL import Image
    from structuredetector_amd.data import FusedOutputDecoder, preprocess_images
    from structuredetector_amd.data.decoders import TtaOutput
    from structuredetector_amd.model.label_nms import LabelNms
    from structuredetector_amd.model.predictor import Predictor
    from structuredetector_amd.model.tta import FlipTta
    from structuredetector_amd.utils import Arguments
    _, common = cli_setup
    args = Arguments().parse(common + ["--label_nms", "3"])
    image = Image.fromarray(np.random.default_rng(4).integers(0, 255, (150, 200, 3), dtype=np.uint8))
    predictor = Predictor(args)
    assert isinstance(predictor.tta, LabelNms) and predictor.tta.net is predictor.model and type(predictor.decoder) is FusedOutputDecoder
    got = predictor(image)
    arr = torch.from_numpy(np.asarray(image.convert("RGB"), np.uint8).copy())[None].to(args.device)
    with torch.no_grad():
        out = predictor.model(preprocess_images(arr, (args.width, args.height)))
    maps = expected_nms5_labels(torch.cat([out["anchor_hm"], out["part_hm"]], 1), 2, 3)
    want = FusedOutputDecoder(args)(TtaOutput(anchor_hm=maps[:, :2], part_hm=maps[:, 2:], offsets=out["offsets"], embeddings=out["embeddings"]))[0]
    assert ann_key(got) == ann_key(want) and len(got.objects) > 0
    both = Predictor(Arguments().parse(common + ["--label_nms", "1", "--tta", "hflip"]))
    assert isinstance(both.tta, LabelNms) and isinstance(both.tta.net, FlipTta) and len(both(image).objects) > 0
    assert Predictor(Arguments().parse(common)).tta is None


def test_detect_cli_with_label_nms_keeps_eval_batch_in_images(cli_setup, monkeypatch):
    from PIL import Image
    from structuredetector_amd.cli import detect
    from structuredetector_amd.model import Network
    tmp_path, common = cli_setup
    (tmp_path / "imgs").mkdir()
    rng = np.random.default_rng(9)
    for i, size in enumerate([(160, 120), (100, 100), (90, 140)]):
        Image.fromarray(rng.integers(0, 255, (size[1], size[0], 3), dtype=np.uint8)).save(tmp_path / "imgs" / f"p{i}.jpg")
    seen = []
    forward = Network.forward

    def spy(self, x):
        seen.append(x.shape[0])
        return forward(self, x)
    monkeypatch.setattr(Network, "forward", spy)
    written = detect.main(common + ["--valid_dir", str(tmp_path / "imgs"), "--eval_batch", "2", "--label_nms", "2"])
    assert [p.name for p in written] == ["p0.json", "p1.json", "p2.json"] and seen == [2, 1]
    with_flag = [json.loads(p.read_text()) for p in written]
    seen.clear()
    written = detect.main(common + ["--valid_dir", str(tmp_path / "imgs"), "--eval_batch", "2", "--label_nms", "2", "--tta", "hflip"])
    assert [p.name for p in written] == ["p0.json", "p1.json", "p2.json"] and seen == [4, 2]
    detect.main(common + ["--valid_dir", str(tmp_path / "imgs"), "--eval_batch", "2"])
    plain = [json.loads(p.read_text()) for p in written]
    assert sum(len(a["objects"]) for a in with_flag) <= sum(len(a["objects"]) for a in plain)
