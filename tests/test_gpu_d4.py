"""Transposed views on the GPU: `sd_d4_views`, `sd_d4_merge_nms` and `sd_transpose_select` bit for bit against their definitions restated
with torch ops (tests/d4_ref.py) and against the CPU oracle, `TransposeTta` + `tta_decoder` end to end, the `--tta_transpose` seams of
`evaluate`, `detect` and `Predictor`, and `--aug_transpose` in `TrainAugmentation`.  Shapes sit around the 64-wide LDS tile."""
import ctypes as C
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.d4_ref import expected_merge, expected_sum, expected_transpose_select, expected_views, flip
from tests.test_gpu_tta import ann_key, cli_setup, default_label_args, evaluator_state  # noqa: F401  (cli_setup: the flip-TTA CLI fixture)

pytestmark = pytest.mark.gpu

FLIPS = {1: (0,), 2: (0, 1), 4: (0, 1, 2, 3)}
VFLIP2 = (0, 2)                                      # the other two-view table
IMAGES = ((5, 30), (32, 32), (64, 64), (96, 160), (130, 70))     # W % 4 != 0; below one tile; one tile; ragged on both axes; H > W, H % 4 != 0
MAPS = ((8, 8), (9, 30), (24, 40), (72, 136), (128, 128))
HM_TOL = 1e-4                                        # the project's standing heatmap tolerance against the CPU oracle


# --------------------------------------------------------------------------------------------- views
@pytest.mark.parametrize("Vf", [1, 2, 4])
@pytest.mark.parametrize("H,W", IMAGES)
def test_views_equal_torch_flips_of_the_image_and_of_its_transpose(H, W, Vf):
    from structuredetector_amd.model.tta import d4_views
    for flips in ((FLIPS[Vf], VFLIP2) if Vf == 2 else (FLIPS[Vf],)):
        for B in (1, 3):
            x = torch.randn(B, 3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(B * H + W))
            want, want_t = expected_views(x, flips)
            out, out_t = d4_views(x, flips)
            assert out.shape == (Vf * B, 3, H, W) and out_t.shape == (Vf * B, 3, W, H)
            assert torch.equal(out, want) and torch.equal(out_t, want_t), (B, flips)
            # separately allocated outputs, straight through the C ABI
            from structuredetector_amd import _lib as L
            a, b = torch.zeros_like(want), torch.zeros_like(want_t)
            L.check(L.lib().sd_d4_views(x.data_ptr(), a.data_ptr(), b.data_ptr(), B, H, W, Vf, (C.c_ubyte * Vf)(*flips), L.stream()), "sd_d4_views")
            assert torch.equal(a, want) and torch.equal(b, want_t), (B, flips)
            if H == W:                               # the contiguous square form: one batch of 2 * Vf * B images
                joint = d4_views(x, flips, joint=True)
                assert joint.shape == (2 * Vf * B, 3, H, W) and torch.equal(joint, torch.cat([want, want_t]))


def test_views_on_pointers_off_16_byte_alignment():
    """Each of the three pointers one float off 16-byte alignment in turn: the 4-byte path of that side, the 16-byte path of the other."""
    from structuredetector_amd import _lib as L
    B, H, W, flips = 2, 96, 160, FLIPS[4]
    x = torch.randn(B, 3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    want, want_t = expected_views(x, flips)
    for which in range(3):
        bufs = [torch.zeros(t.numel() + 1, device="cuda") for t in (x, want, want_t)]
        views = [buf[(1 if k == which else 0):][:t.numel()].view(t.shape) for k, (buf, t) in enumerate(zip(bufs, (x, want, want_t)))]
        views[0].copy_(x)
        assert views[which].data_ptr() % 16 == 4
        L.check(L.lib().sd_d4_views(views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(), B, H, W, 4, (C.c_ubyte * 4)(*flips), L.stream()),
                "sd_d4_views")
        assert torch.equal(views[1], want) and torch.equal(views[2], want_t), which


def test_direction_of_the_transposed_views():
    """A one-hot image at (y, x) lands at row x, column y of the transposed view, at column H-1-y under its hflip and at row W-1-x under its vflip."""
    from structuredetector_amd.model.tta import d4_views
    H, W, y, x = 70, 130, 3, 101
    img = torch.zeros(1, 3, H, W, device="cuda")
    img[0, :, y, x] = 1.0
    out, out_t = d4_views(img, FLIPS[4])
    where = lambda t: [tuple(p) for p in t[0, 1].nonzero().tolist()]      # (one channel: the three are alike)
    assert [where(out[v:v + 1]) for v in range(4)] == [[(y, x)], [(y, W - 1 - x)], [(H - 1 - y, x)], [(H - 1 - y, W - 1 - x)]]
    assert [where(out_t[v:v + 1]) for v in range(4)] == [[(x, y)], [(x, H - 1 - y)], [(W - 1 - x, y)], [(W - 1 - x, H - 1 - y)]]


# --------------------------------------------------------------------------------------------- merge
@functools.lru_cache(maxsize=None)
def merge_case(h, w, Cc, B, Vf):
    """(plain logits (Vf*B, C, h, w), transposed logits (Vf*B, C, w, h) on the host, expected merged map on the GPU); shared, never modified."""
    g = torch.Generator().manual_seed(1000 * h + 10 * w + 3 * Cc + B + Vf)
    x = torch.randn(Vf * B, Cc, h, w, generator=g) * 4
    xt = torch.randn(Vf * B, Cc, w, h, generator=g) * 4
    for t in (x, xt):
        flat = t.view(-1)
        hit = torch.randperm(flat.numel(), generator=g)[:8]
        flat[hit[:4]], flat[hit[4:]] = 30.0, -30.0                   # both clamps
    return x, xt, expected_merge(x.cuda(), xt.cuda(), FLIPS[Vf])


@pytest.mark.parametrize("Vf", [1, 2, 4])
@pytest.mark.parametrize("h,w", MAPS)
def test_merge_bitwise_on_contiguous_planes(h, w, Vf):
    from structuredetector_amd.model.tta import d4_merge_nms
    for Cc in (1, 5):
        for B in (1, 3):
            x, xt, want = merge_case(h, w, Cc, B, Vf)
            got = d4_merge_nms(x.cuda(), xt.cuda(), FLIPS[Vf])
            assert got.shape == (B, Cc, h, w)
            assert torch.equal(got, want), f"C={Cc} B={B}: {(got != want).sum().item()} of {want.numel()} values differ"
            assert (got > 0).any() and (got == 0).any()


@pytest.mark.parametrize("h,w", [(24, 40), (40, 24), (9, 30), (30, 9), (12, 30), (30, 12), (20, 70), (70, 20)])      # (12, 30): 16-byte loads on the transposed side only; (30, 12): on the plain side only
def test_merge_bitwise_with_the_vertical_two_view_table(h, w):
    from structuredetector_amd.model.tta import d4_merge_nms
    g = torch.Generator().manual_seed(h * 100 + w)
    x, xt = (torch.randn(4, 3, h, w, generator=g) * 4).cuda(), (torch.randn(4, 3, w, h, generator=g) * 4).cuda()
    assert torch.equal(d4_merge_nms(x, xt, VFLIP2), expected_merge(x, xt, VFLIP2))


@pytest.mark.parametrize("Vf", [1, 2, 4])
@pytest.mark.parametrize("h,w", MAPS)
def test_merge_bitwise_on_channel_slice_views(h, w, Vf):
    """The heatmap channels as a slice (from channel 1) of (Vf*B, C + 4, ., .) head tensors: strided planes, consumed in place."""
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model.tta import d4_merge_nms
    for Cc in (1, 5):
        for B in (1, 3):
            x, xt, want = merge_case(h, w, Cc, B, Vf)
            head, head_t = torch.randn(Vf * B, Cc + 4, h, w, device="cuda"), torch.randn(Vf * B, Cc + 4, w, h, device="cuda")
            head[:, 1:1 + Cc], head_t[:, 1:1 + Cc] = x.cuda(), xt.cuda()
            view, view_t = head[:, 1:1 + Cc], head_t[:, 1:1 + Cc]
            if h * w % 4 == 0:                       # consumed in place (a plane of 9 x 30 floats leaves channel 1 off 16-byte alignment: `map_view` copies)
                assert L.map_view(view)[1] == view.data_ptr() and L.map_view(view_t)[1] == view_t.data_ptr()
            assert torch.equal(d4_merge_nms(view, view_t, FLIPS[Vf]), want), f"C={Cc} B={B}"


@pytest.mark.parametrize("Vf", [1, 2, 4])
def test_merge_bitwise_on_pointers_off_16_byte_alignment(Vf):
    """Either map one float off 16-byte alignment (straight through the C ABI; `map_view` would copy it): the 4-byte loads of that side."""
    from structuredetector_amd import _lib as L
    h, w, Cc, B = 24, 40, 5, 3
    x, xt, want = merge_case(h, w, Cc, B, Vf)
    for which in range(2):
        bufs = [torch.empty(t.numel() + 1, device="cuda") for t in (x, xt)]
        views = [buf[(1 if k == which else 0):][:t.numel()].view(t.shape) for k, (buf, t) in enumerate(zip(bufs, (x, xt)))]
        views[0].copy_(x), views[1].copy_(xt)
        assert views[which].data_ptr() % 16 == 4 and views[1 - which].data_ptr() % 16 == 0
        out = torch.empty_like(want)
        L.check(L.lib().sd_d4_merge_nms(views[0].data_ptr(), views[0].stride(0), views[0].stride(1), views[1].data_ptr(), views[1].stride(0),
                                        views[1].stride(1), out.data_ptr(), B, Cc, h, w, Vf, (C.c_ubyte * Vf)(*FLIPS[Vf]), L.stream()),
                "sd_d4_merge_nms")
        assert torch.equal(out, want), which


@pytest.mark.parametrize("Vf", [1, 2, 4])
@pytest.mark.parametrize("h,w", MAPS)
def test_merge_against_the_cpu_oracle(h, w, Vf):
    """The same inputs through the oracle's clamped_sigmoid / nms on the CPU: values within the standing 1e-4, and (tie-free inputs) the
    same set of surviving positions."""
    from oracle import sdnet_oracle as O
    from structuredetector_amd.model.tta import d4_merge_nms
    sigmoid = lambda t: torch.from_numpy(O.clamped_sigmoid(t.numpy()))
    for Cc in (1, 5):
        for B in (1, 3):
            x, xt, _ = merge_case(h, w, Cc, B, Vf)
            ref = O.nms(expected_sum(x, xt, FLIPS[Vf], sigmoid).contiguous().numpy())
            got = d4_merge_nms(x.cuda(), xt.cuda(), FLIPS[Vf]).cpu().numpy()
            print(f"h={h} w={w} C={Cc} B={B} Vf={Vf}: max |got - oracle| = {np.abs(got - ref).max():.3e}, "
                  f"survivors {int((got > 0).sum())} vs {int((ref > 0).sum())}")
            np.testing.assert_allclose(got, ref, rtol=0, atol=HM_TOL)
            np.testing.assert_array_equal(got != 0, ref != 0)


def test_views_of_one_map_merge_to_the_plain_map():
    """Every view the exact image of view 0 under its symmetry: the two four-term sums and their sum times 1/8 are exact."""
    from structuredetector_amd.model.tta import d4_merge_nms
    from structuredetector_amd.utils import clamped_sigmoid, nms
    x0 = torch.randn(3, 5, 72, 136, device="cuda", generator=torch.Generator("cuda").manual_seed(5)) * 4
    plain, transposed = expected_views(x0, FLIPS[4])
    assert torch.equal(d4_merge_nms(plain, transposed, FLIPS[4]), nms(clamped_sigmoid(x0)))


# --------------------------------------------------------------------------------------------- transpose_select
@pytest.mark.parametrize("S", [1, 5, 33, 64, 96])
def test_transpose_select_equals_torch(S):
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data.augment import transpose_select
    B, P = 4, 3
    x = torch.randn(B, P, S, S, device="cuda", generator=torch.Generator("cuda").manual_seed(S))
    for sel in ([0, 0, 0, 0], [1, 1, 1, 1], [0, 1, 1, 0], [0xFE, 0x81, 0x03, 0x40]):        # the last: high bits set, bit 0 decides
        got = transpose_select(x, sel)
        assert got.data_ptr() != x.data_ptr() and torch.equal(got, expected_transpose_select(x, sel)), sel
    # a pointer 4 bytes off 16-byte alignment: the 4-byte path whatever S is
    buf = torch.empty(x.numel() + 1, device="cuda")
    off = buf[1:].view(x.shape)
    off.copy_(x)
    out = torch.empty_like(x)
    sel = torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device="cuda")
    L.check(L.lib().sd_transpose_select(off.data_ptr(), out.data_ptr(), B, P, S, sel.data_ptr(), L.stream()), "sd_transpose_select")
    assert torch.equal(out, expected_transpose_select(x, sel.tolist()))


# --------------------------------------------------------------------------------------------- end to end
def compose(net, x, flips, M, N):
    """The hand composition: the same batches built with torch ops, the same forwards, the d4_ref merge, view 0's regressions."""
    B = x.shape[0]
    n = len(flips) * B
    plain, transposed = expected_views(x, flips)
    with torch.no_grad():
        if x.shape[2] == x.shape[3]:
            out = net(torch.cat([plain, transposed]))
            heat = torch.cat([out["anchor_hm"], out["part_hm"]], 1)
            heat, heat_t = heat[:n], heat[n:]
        else:
            out, out_t = net(plain), net(transposed)
            heat, heat_t = torch.cat([out["anchor_hm"], out["part_hm"]], 1), torch.cat([out_t["anchor_hm"], out_t["part_hm"]], 1)
    merged = expected_merge(heat, heat_t, flips)
    return {"anchor_hm": merged[:, :M], "part_hm": merged[:, M:], "offsets": out["offsets"][:B], "embeddings": out["embeddings"][:B]}


@pytest.mark.parametrize("mode", ["none", "hvflip"])
@pytest.mark.parametrize("H,W", [(64, 64), (64, 96)])
def test_transpose_tta_on_a_random_network_equals_the_composition(H, W, mode):
    from structuredetector_amd.data import FusedOutputDecoder
    from structuredetector_amd.data.decoders import TtaOutput
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.tta import VIEW_FLIPS, TransposeTta, tta_decoder
    args = default_label_args()
    M, N = len(args.labels), len(args.parts)
    flips = VIEW_FLIPS.get(mode, (0,))
    torch.manual_seed(11)
    net = Network(args, pretrained=False).cuda().eval()
    x = torch.randn(2, 3, H, W, device="cuda")
    seen = []
    handle = net.register_forward_pre_hook(lambda mod, inp: seen.append(tuple(inp[0].shape)))
    with torch.no_grad():
        got = TransposeTta(net, args, mode)(x)
    handle.remove()
    n = 2 * len(flips)
    assert seen == ([(2 * n, 3, H, W)] if H == W else [(n, 3, H, W), (n, 3, W, H)])       # one forward when square, two otherwise
    want = compose(net, x, flips, M, N)
    assert isinstance(got, TtaOutput) and set(got) == {"anchor_hm", "part_hm", "offsets", "embeddings"}
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert got["anchor_hm"].shape == (2, M, H // 4, W // 4)
    # view 0's regression channels are views into the head tensor of the forward that held view 0: no copy
    assert got["offsets"].untyped_storage().data_ptr() == got["embeddings"].untyped_storage().data_ptr()
    images = 2 * n if H == W else n
    assert got["offsets"].untyped_storage().nbytes() >= images * (M + N + 4) * (H // 4) * (W // 4) * 4
    for conf in (None, 0.0):
        a, b = tta_decoder(args)(got, conf_thresh=conf), FusedOutputDecoder(args)(want, conf_thresh=conf)
        assert [ann_key(i) for i in a] == [ann_key(i) for i in b]
    assert sum(len(i) for i in a) > 0


# --------------------------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("extra,mode", [([], "none"), (["--tta", "hflip"], "hflip")])
def test_evaluate_cli_with_tta_transpose(cli_setup, capsys, extra, mode):
    from structuredetector_amd.cli import evaluate
    from structuredetector_amd.data import FusedOutputDecoder
    from structuredetector_amd.data.synthetic import synthetic_samples
    from structuredetector_amd.model import Evaluator, Network
    from structuredetector_amd.model.tta import VIEW_FLIPS
    _, common = cli_setup
    argv = common + ["--synthetic", "8"]
    ev = evaluate.main(argv + ["--tta_transpose"] + extra)
    assert "Anchor Location" in capsys.readouterr().out
    args = evaluate.Arguments().parse(argv)
    net = Network(args, pretrained=False, init_weights=False)
    net.load_state_dict(torch.load(args.pretrained_model, map_location="cpu", weights_only=True))
    net = net.eval().to(args.device)
    want, dec = Evaluator(args), FusedOutputDecoder(args)
    for image, annotation in synthetic_samples(args, 8):
        data = dec(compose(net, image[None], VIEW_FLIPS.get(mode, (0,)), 2, 1), return_metadata=True, metadata_fields=("annotation", "raw_parts"))
        want.accumulate(data["annotation"][0], annotation, data["raw_parts"][0], True, True)
    assert evaluator_state(ev) == evaluator_state(want)
    assert ev.anchor_eval.reduce().npos > 0 and ev.anchor_eval.reduce().ndet > 0


@pytest.mark.parametrize("extra,mode", [([], "none"), (["--tta", "hflip"], "hflip")])
def test_predictor_with_tta_transpose(cli_setup, extra, mode):
    from PIL import Image
    from structuredetector_amd.data import FusedOutputDecoder, preprocess_images
    from structuredetector_amd.model.predictor import Predictor
    from structuredetector_amd.model.tta import VIEW_FLIPS, TransposeTta
    from structuredetector_amd.utils import Arguments
    _, common = cli_setup
    args = Arguments().parse(common + ["--tta_transpose"] + extra)
    image = Image.fromarray(np.random.default_rng(4).integers(0, 255, (150, 200, 3), dtype=np.uint8))
    predictor = Predictor(args)
    assert isinstance(predictor.tta, TransposeTta) and predictor.tta.mode == mode and isinstance(predictor.decoder, FusedOutputDecoder)
    got = predictor(image)
    arr = torch.from_numpy(np.asarray(image.convert("RGB"), np.uint8).copy())[None].to(args.device)
    with torch.no_grad():
        x = preprocess_images(arr, (args.width, args.height))
    want = FusedOutputDecoder(args)(compose(predictor.model, x, VIEW_FLIPS.get(mode, (0,)), 2, 1))[0]
    assert ann_key(got) == ann_key(want) and len(got.objects) > 0


@pytest.mark.parametrize("extra,mode", [([], "none"), (["--tta", "hflip"], "hflip")])
def test_detect_cli_with_tta_transpose_keeps_eval_batch_in_images(cli_setup, monkeypatch, extra, mode):
    """`--eval_batch` counts images: the forward sees 2 * Vf times as many, also for the ragged last batch (3 images at 2); the written
    annotations are those of the hand composition."""
    from PIL import Image
    from structuredetector_amd.cli import detect
    from structuredetector_amd.data import FusedOutputDecoder, preprocess_images
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.tta import VIEW_FLIPS
    from structuredetector_amd.utils import Arguments
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
    flips = VIEW_FLIPS.get(mode, (0,))
    written = detect.main(common + ["--valid_dir", str(tmp_path / "imgs"), "--eval_batch", "2", "--tta_transpose"] + extra)
    assert [p.name for p in written] == ["p0.json", "p1.json", "p2.json"] and seen == [4 * len(flips), 2 * len(flips)]
    monkeypatch.setattr(Network, "forward", forward)
    args = Arguments().parse(common)
    net = Network(args, pretrained=False, init_weights=False)
    net.load_state_dict(torch.load(args.pretrained_model, map_location="cpu", weights_only=True))
    net = net.eval().to(args.device)
    (tmp_path / "want").mkdir()
    for batch in ([0, 1], [2]):                                                     # the batches `detect` ran
        paths = [tmp_path / "imgs" / f"p{i}.jpg" for i in batch]
        images = [Image.open(p).convert("RGB") for p in paths]
        with torch.no_grad():
            x = torch.cat([preprocess_images(torch.from_numpy(np.asarray(im, np.uint8).copy())[None].to(args.device), (args.width, args.height))
                           for im in images])
        for ann, image, path in zip(FusedOutputDecoder(args)(compose(net, x, flips, 2, 1)), images, paths):
            ann.resize((args.width, args.height), image.size)
            ann.img_size, ann.image_path = image.size, path
            ann.save_json(tmp_path / "want")
            name = path.with_suffix(".json").name
            assert (tmp_path / "want" / name).read_text() == (tmp_path / "predictions" / name).read_text(), name


# --------------------------------------------------------------------------------------------- training
def _ann_rows(a):
    return [(o.name, o.x, o.y, [(p.kind, p.x, p.y) for p in o.parts],
             None if o.box is None else (o.box.x_min, o.box.y_min, o.box.x_max, o.box.y_max)) for o in a.objects]


def test_train_augmentation_with_aug_transpose(golden_dir, tmp_path):
    """P = 1: the batch is the transpose of the P = 0 batch of the same draws and the annotations are `transpose_annotation` of that run's;
    P = 0.5: the per-image choice follows the drawn bits; the device image cache gives the same batch."""
    from structuredetector_amd.data import BatchFeeder, CropDataset, DeviceImageCache, TrainAugmentation
    from structuredetector_amd.utils.misc import clip_annotation, transpose_annotation
    from tests.helpers import EVAL16_LABELS, EVAL16_PARTS, write_evaluate16_dir
    write_evaluate16_dir(np.load(golden_dir / "evaluate16.npz"), tmp_path / "train")
    dev = torch.device("cuda", torch.cuda.current_device())
    common = dict(labels=EVAL16_LABELS, parts=EVAL16_PARTS, width=128, height=128, anchor_name="stem", device=dev, no_augmentation=False,
                  aug_rotate=15.0)
    ds = CropDataset(Namespace(**common), tmp_path / "train", raw=True)
    picks = [0, 1, 2, 3, 5, 8, 13, 4]
    n = len(picks)

    def run(p, cache=None):
        batch = next(iter(BatchFeeder(ds, [picks], "cuda", workers=2, cache=cache)))      # fresh annotations: the augmentation edits them in place
        torch.manual_seed(31)
        return TrainAugmentation(Namespace(**common, aug_transpose=p))(batch, batch.annotations)

    saved = torch.get_rng_state()
    try:
        base, base_anns = run(0.0)
        state0 = torch.get_rng_state()
        bits = (torch.rand(n, dtype=torch.float64) < 0.5).tolist()                        # the one more draw, after all the others
        state1 = torch.get_rng_state()
        assert 0 < sum(bits) < n
        full, full_anns = run(1.0)
        assert torch.equal(torch.get_rng_state(), state1)                                 # exactly rand(n) in float64 more than P = 0
        assert full.shape == base.shape == (n, 3, 128, 128) and torch.equal(full, base.transpose(-1, -2))
        assert not torch.equal(full, base)
        want = [_ann_rows(clip_annotation(transpose_annotation(a, (128, 128)), (128, 128))) for a in run(0.0)[1]]
        assert torch.equal(torch.get_rng_state(), state0)
        assert [_ann_rows(a) for a in full_anns] == want and want != [_ann_rows(a) for a in base_anns]
        half, half_anns = run(0.5)
        for i in range(n):
            assert torch.equal(half[i], base[i].transpose(-1, -2) if bits[i] else base[i]), i
            assert _ann_rows(half_anns[i]) == (want[i] if bits[i] else _ann_rows(base_anns[i])), i
        cache = DeviceImageCache(1 << 28, "cuda")
        cache.prefill(ds, workers=2)
        cached, cached_anns = run(0.5, cache)
        assert torch.equal(cached, half) and [_ann_rows(a) for a in cached_anns] == [_ann_rows(a) for a in half_anns]
    finally:
        torch.set_rng_state(saved)
