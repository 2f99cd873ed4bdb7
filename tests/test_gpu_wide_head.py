"""Wide heads on the GPU: 33 .. 256 output channels (up to 252 labels + parts).  The GEMM head kernels of sd_head_wide.hip against
F.conv2d and its autograd, then every layer that sees M + N -- the network, the mixed-precision step, Encode, the loss, the decoder
(map-parallel path and launch pair) and the train / evaluate / fused-export entry points -- at label counts the narrow head refused."""
import copy
import json
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sdnet_oracle as O
from tests.helpers import ENC_KEYS, assert_decode_matches_oracle
from tests.test_gpu_network import close, from_nhwc, nhwc
from tests.test_host_cpu import make_args, to_annotation

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIG_TOL = dict(rtol=4e-7, atol=0)
SD_ERR_INVALID = -1
WIDE_CASES = [(2, 48, 48, 128, 33), (3, 64, 80, 128, 64), (1, 45, 37, 64, 100), (2, 32, 32, 256, 132), (1, 128, 128, 128, 256)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def head_views(head, M, N):
    return {"anchor_hm": head[:, :M], "part_hm": head[:, M:M + N], "offsets": head[:, M + N:M + N + 2],
            "embeddings": head[:, M + N + 2:M + N + 4]}


@pytest.mark.parametrize("B,H,W,C,Co", WIDE_CASES)
def test_wide_head_kernels_vs_conv2d(B, H, W, C, Co):
    """sd_head_fwd / sd_head_fwd_bf16 / sd_head_bwd at Co > 32 against F.conv2d and its autograd on the CPU (fp32 products and sums in
    another order: 1e-5 of the largest value); accumulate 0 then 1; repeated backward calls give the same bits."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    g = torch.Generator().manual_seed(B * 1000 + Co)
    xh = torch.randn(B, C, H, W, generator=g).requires_grad_(True)
    wh = (torch.randn(Co, C, 1, 1, generator=g) / C ** 0.5).requires_grad_(True)
    bh = torch.randn(Co, generator=g).requires_grad_(True)
    yh = F.conv2d(xh, wh, bh)
    dyh = torch.randn(yh.shape, generator=g)
    yh.backward(dyh)
    x_d = nhwc(xh.detach())
    whd = wh.detach().reshape(Co, C).to(DEV).contiguous(); bhd = bh.detach().to(DEV)
    out = torch.full((B, Co, H, W), float("nan"), device=DEV)
    L.check(lib.sd_head_fwd(x_d.data_ptr(), whd.data_ptr(), bhd.data_ptr(), out.data_ptr(), B, H * W, C, Co, L.stream()), "sd_head_fwd")
    close(out.cpu(), yh.detach(), 1e-5)
    # bf16 activation, fp32 weights: against the fp32 conv of the bf16-rounded input
    x16 = x_d.to(torch.bfloat16)
    want16 = F.conv2d(xh.detach().to(torch.bfloat16).float(), wh.detach(), bh.detach())
    out.fill_(float("nan"))
    L.check(lib.sd_head_fwd_bf16(x16.data_ptr(), whd.data_ptr(), bhd.data_ptr(), out.data_ptr(), B, H * W, C, Co, L.stream()), "sd_head_fwd_bf16")
    close(out.cpu(), want16, 1e-5)
    # backward
    nws = lib.sd_head_bwd_workspace_bytes(B, H * W, C, Co)
    assert nws <= 64 << 20
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    dy_d = dyh.to(DEV)
    dx = torch.full((B, H, W, C), float("nan"), device=DEV)
    dw = torch.full((Co, C), float("nan"), device=DEV); db = torch.full((Co,), float("nan"), device=DEV)
    for acc in (0, 1):
        L.check(lib.sd_head_bwd(dy_d.data_ptr(), x_d.data_ptr(), whd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                B, H * W, C, Co, acc, ws.data_ptr(), ws.numel(), L.stream()), "sd_head_bwd")
        close(from_nhwc(dx), xh.grad, 1e-5)
        close(dw.cpu(), (1 + acc) * wh.grad.reshape(Co, C), 1e-5)
        close(db.cpu(), (1 + acc) * bh.grad, 1e-5)
    dw2 = torch.empty_like(dw); db2 = torch.empty_like(db)
    for a, b in ((dw2, db2), (dw, db)):
        L.check(lib.sd_head_bwd(dy_d.data_ptr(), x_d.data_ptr(), whd.data_ptr(), dx.data_ptr(), a.data_ptr(), b.data_ptr(),
                                B, H * W, C, Co, 0, ws.data_ptr(), ws.numel(), L.stream()), "sd_head_bwd")
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


def test_wide_head_unsupported_depth_is_rejected():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    x = torch.zeros(1, 8, 8, 96, device=DEV); w = torch.zeros(40, 96, device=DEV); b = torch.zeros(40, device=DEV)
    y = torch.zeros(1, 40, 8, 8, device=DEV)
    assert lib.sd_head_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, 64, 96, 40, L.stream()) == SD_ERR_INVALID
    assert lib.sd_head_fwd_bf16(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, 64, 96, 40, L.stream()) == SD_ERR_INVALID
    ws = torch.empty(lib.sd_head_bwd_workspace_bytes(1, 64, 96, 40), dtype=torch.uint8, device=DEV)
    assert lib.sd_head_bwd(y.data_ptr(), x.data_ptr(), w.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), 1, 64, 96, 40, 0,
                           ws.data_ptr(), ws.numel(), L.stream()) == SD_ERR_INVALID
    torch.cuda.synchronize()
    assert float(y.abs().sum()) == 0.0


def _pair(M, N, seed, **kw):
    from structuredetector_amd.model import Network
    ref = O.build_reference_network(M, N, seed=seed)
    args = Namespace(labels={f"l{i}": i for i in range(M)}, parts={f"p{i}": i for i in range(N)}, fpn_depth=128, **kw)
    net = Network(args, pretrained=False, raw_output=True)
    net.load_state_dict(ref.state_dict())
    return ref, net.to(DEV)


@pytest.mark.parametrize("M,N", [(30, 20), (100, 60)])
def test_wide_network_fp32_vs_oracle(M, N):
    """fp32 eval forward (B = 2, 256 x 256) and one training forward + backward (B = 2, 128 x 192) against the oracle network."""
    ref, net = _pair(M, N, seed=M + N)
    g = torch.Generator().manual_seed(M)
    x = torch.randn(2, 3, 256, 256, generator=g)
    with torch.no_grad():
        want = ref.eval()(x)
        got = net.eval()(x.to(DEV))
    assert got.shape == want.shape == (2, M + N + 4, 64, 64)
    close(got.cpu(), want, 1e-4)
    x = torch.randn(2, 3, 128, 192, generator=g)
    dy = torch.randn(2, M + N + 4, 32, 48, generator=g)
    ref.train(); net.train()
    want = ref(x)
    want.backward(dy)
    got = net(x.to(DEV))
    got.backward(dy.to(DEV))
    close(got.detach().cpu(), want.detach(), 1e-4)
    sd_ref = dict(ref.named_parameters())
    # the head's own gradients (the wide kernels' weight-gradient reduction) at 1e-4 of the largest value
    close(net.head.conv.weight.grad.cpu(), sd_ref["head.conv.weight"].grad, 1e-4)
    close(net.head.conv.bias.grad.cpu(), sd_ref["head.conv.bias"].grad, 1e-4)
    # everything upstream of the head's data gradient runs the narrow network's kernels through 44 BN-coupled fp32 layers with a batch of
    # 2: an input within an ulp of a ReLU's zero may land on the other side in one of the two implementations and move the deep, small-map
    # tensors (down4: 4 x 6 pixels) by percents (see test_network_train_forward_backward, which needed a seed search at 2e-3).  So the
    # whole gradient is held by direction, as test_amp_step_at_odd_batches_and_non_square_inputs does, and every tensor must be finite.
    got_all, ref_all = [], []
    for name, p in net.named_parameters():
        gr, gg = sd_ref[name].grad, p.grad.cpu()
        assert gg.shape == gr.shape and torch.isfinite(gg).all(), name
        got_all.append(gg.flatten().double()); ref_all.append(gr.flatten().double())
    cos = F.cosine_similarity(torch.cat(got_all), torch.cat(ref_all), dim=0).item()
    assert cos > 0.999, cos


@pytest.mark.parametrize("M,N", [(30, 20), (100, 60)])
def test_wide_network_bf16_inference_and_amp_step_vs_oracle(M, N):
    """bf16 inference forward against the oracle under autocast; the mixed-precision step against an fp64 run of the oracle (as close to it
    as the autocast oracle is: error populations over all parameter tensors within a factor 2)."""
    ref, net = _pair(M, N, seed=2 * M + N, use_amp=True)
    g = torch.Generator().manual_seed(N)
    x = torch.randn(2, 3, 256, 256, generator=g)
    ref.eval(); net.eval()
    with torch.no_grad():
        want32 = ref(x)
        with torch.autocast(device_type="cpu", dtype=torch.bfloat16):
            want16 = ref(x).float()
        got = net(x.to(DEV)).cpu()
    assert got.dtype == torch.float32 and got.shape == want32.shape
    scale = want32.abs().max().item()
    err_ours = (got - want32).abs().max().item() / scale
    err_autocast = (want16 - want32).abs().max().item() / scale
    assert err_ours <= max(1.5 * err_autocast, 2e-2), (err_ours, err_autocast)
    # AMP step
    x = torch.randn(4, 3, 128, 128, generator=g)
    dy = torch.randn(4, M + N + 4, 32, 32, generator=g) * 0.1
    ref.train(); net.train()
    ref64 = copy.deepcopy(ref).double()
    ref_ac = copy.deepcopy(ref)
    out64 = ref64(x.double()); out64.backward(dy.double())
    with torch.autocast(device_type="cpu", dtype=torch.bfloat16):
        out_ac = ref_ac(x)
    out_ac.float().backward(dy)
    out, tape = net.forward_train(x.to(DEV), amp=True)
    assert tape["amp"] is True and tape["f1"].dtype == torch.bfloat16
    net.backward_from(tape, dy.to(DEV))
    scale = out64.abs().max().item()
    e_fwd_gpu = (out.cpu().double() - out64.detach()).abs().max().item() / scale
    e_fwd_ac = (out_ac.detach().double() - out64.detach()).abs().max().item() / scale
    assert e_fwd_gpu <= 2 * e_fwd_ac + 1e-3, (e_fwd_gpu, e_fwd_ac)
    g64, gac = dict(ref64.named_parameters()), dict(ref_ac.named_parameters())
    e_gpu, e_ac = [], []
    for name, p in net.named_parameters():
        truth = g64[name].grad
        s = truth.abs().max().item() + 1e-30
        e_gpu.append((net.grad_of(p).cpu().double() - truth).abs().max().item() / s)
        e_ac.append((gac[name].grad.double() - truth).abs().max().item() / s)
    e_gpu, e_ac = np.array(e_gpu), np.array(e_ac)
    assert np.isfinite(e_gpu).all()
    assert np.median(e_gpu) <= 2 * np.median(e_ac) + 1e-3, (np.median(e_gpu), np.median(e_ac))
    assert np.mean(e_gpu) <= 2 * np.mean(e_ac) + 1e-3, (np.mean(e_gpu), np.mean(e_ac))
    assert e_gpu.max() <= 2 * e_ac.max() + 1e-2, (e_gpu.max(), e_ac.max())


@pytest.mark.parametrize("hm_fn", ["mse", "focal"])
def test_wide_encode_and_loss_vs_oracle(hm_fn):
    from structuredetector_amd.data import Encode
    from structuredetector_amd.model import Loss
    M, N, K, P, W, H = 40, 30, 20, 40, 128, 128
    args = make_args(M, N, K, P, device=torch.device(DEV), hm_loss_fn=hm_fn)
    rng = np.random.default_rng(40)
    scenes = [O.synthetic_scene(rng, W, H, M, N, 3, 8) for _ in range(3)]
    out = Encode(args).batch((W, H), [to_annotation(args, s, f"img{i}.png") for i, s in enumerate(scenes)])
    want = O.collate([O.encode(W, H, s, M, N, K, P, 4.0, 0.1) for s in scenes])
    for k in ENC_KEYS:
        got = out[k].cpu().numpy()
        assert got.shape == want[k].shape and got.dtype == want[k].dtype, k
        if k.endswith("_hm"):
            np.testing.assert_allclose(got, want[k], rtol=1e-5, atol=1e-7, err_msg=k)
        else:
            np.testing.assert_array_equal(got, want[k], err_msg=k)
    head = rng.standard_normal((3, M + N + 4, H // 4, W // 4)).astype(np.float32)
    ref = O.loss(head, want, M, N, hm_loss_fn=hm_fn, want_grad=True)
    hd = dev(head).requires_grad_(True)
    crit = Loss(args)
    val = crit(head_views(hd * 1.0, M, N), out)
    val.backward()
    np.testing.assert_allclose([val.item(), float(crit.stats.hm_loss), float(crit.stats.offset_loss), float(crit.stats.embedding_loss)],
                               [ref["total"], ref["hm"], ref["offset"], ref["embedding"]], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(hd.grad.cpu().numpy(), ref["grad"], rtol=1e-4, atol=1e-4 * np.abs(ref["grad"]).max())


@pytest.mark.parametrize("M,N", [(30, 20), (70, 70)])
def test_wide_decoder_vs_oracle(M, N):
    """(30, 20): the map-parallel path; (70, 70): past its 64 + 64 maps, the launch pair.  exact_topk 0 / 1, fused None / False."""
    from structuredetector_amd.data import Decoder
    B, img, K, P = 2, 256, 20, 40
    rng = np.random.default_rng(M * N)
    heads = [O.head_from_targets(rng, O.encode(img, img, O.synthetic_scene(rng, img, img, M, N, 3, 8), M, N, K, P, 4.0, 0.1), M, N, noise=0.3)
             for _ in range(B)]
    head = np.stack(heads)
    t = O.decode_tensors(head[:, :M], head[:, M:M + N], head[:, M + N:M + N + 2], head[:, M + N + 2:], K, P, 0.5, 0.1)
    dec = Decoder(make_args(M, N, K, P))
    views = head_views(dev(head), M, N)
    for exact in (False, True):
        for fused in (None, False):
            packed, _ = dec.decode_packed(views, 0.5, 0.1, exact_topk=exact, fused=fused)
            got = dec.split_packed(packed.cpu().numpy(), B, K, P)
            if exact:
                checked, total, _ = assert_decode_matches_oracle(got, t, 0.5, SIG_TOL)
                assert checked >= 0.9 * total and t["valid"].sum() > 0, (exact, fused, checked, total)
            else:       # ranks are defined down to the score threshold only (early score cut): the peaks above it, as smoke() checks
                for grp in ("anchor", "part"):
                    pos = t[f"{grp}_out"][..., 2] > 0.5
                    assert pos.sum() > 0
                    np.testing.assert_array_equal(got[f"{grp}_ind"][pos], t[f"{grp}_inds"][pos], err_msg=f"{grp} fused={fused}")


def test_wide_train_evaluate_and_fused_export(tmp_path, monkeypatch, capsys):
    """40 labels + 30 parts through `train` and `evaluate`, then the fused export against Network + Decoder on the same forward."""
    from structuredetector_amd.cli import evaluate, train
    from structuredetector_amd.data import Decoder, FusedOutputDecoder
    from structuredetector_amd.model import FusedInferenceModel, Network
    monkeypatch.chdir(tmp_path)
    M, N = 40, 30
    labels = [f"plant{i}" for i in range(M)]
    parts = [f"part{i}" for i in range(N)]
    (tmp_path / "labels.json").write_text(json.dumps({"labels": labels, "parts": parts}))
    common = ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json")]
    train.main(common + ["--synthetic", "8", "-b", "4", "--steps", "3"])
    ckpts = list((tmp_path / "trainings").glob("*/model_best_loss.pth"))
    assert len(ckpts) == 1
    sd = torch.load(ckpts[0], map_location="cpu")
    assert sd["head.conv.weight"].shape == (M + N + 4, 128, 1, 1)
    capsys.readouterr()
    evaluate.main(common + ["--synthetic", "3", "-o", str(ckpts[0])])
    out = capsys.readouterr().out
    assert "Anchor Location" in out and "CSI" in out and "Classification" in out
    # fused export: same annotations as Network + Decoder
    args = make_args(M, N, 20, 40, device=torch.device(DEV))
    net = Network(args, pretrained=False).to(DEV).eval()
    net.load_state_dict(sd)
    fused = FusedInferenceModel(net, args)
    x = torch.randn(1, 3, 128, 160, device=DEV)
    with torch.no_grad():
        f = fused(x)
        logits = net(x)
    assert f.shape == (1, M + N + 4, 32, 40)
    a1 = Decoder(args)(head_views(logits, M, N))
    a2 = FusedOutputDecoder(args)(fused.split(f))
    key = lambda anns: [[(o.name, o.x, o.y, o.anchor.score, [(p.kind, p.x, p.y, p.score) for p in o.parts]) for o in a.objects] for a in anns]
    assert key(a1) == key(a2)
