"""Fine-tuning with frozen trunk stages and frozen BatchNorm (`Network.freeze`, `train --freeze_stages N [--freeze_bn]`) on the GPU.

The kernel (sd_frozen_bn_bwd / sd_frozen_bn_bwd_bf16) is a pure function of its inputs and is held bit for bit against the torch
expression of its definition.  The engine is held against the oracle network with the same stages in `.eval()` / `requires_grad_(False)`,
by the yardsticks of tests/test_gpu_network.py (fp32) and tests/test_gpu_amp.py (mixed precision).  Every oracle run is made once per
(geometry, N, frozen BatchNorm) and shared."""
import copy
import ctypes as C
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import sdnet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
STAGES = ("adpater", "down1", "down2", "down3", "down4")


def close(got, ref, tol):
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, f"max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- the kernel, bit for bit ---------------------------------------------------------------------------------------------------------------
GUARD = 64              # elements behind every output that the launch must leave alone


def _shifted(t, off):
    """a copy of `t` whose data pointer is `off` elements past an allocation's (16-byte aligned) start"""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    view = buf[off:].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,Cc", [(1, 64), (30, 64), (4099, 64), (77, 512), (1025, 128)])
def test_frozen_bn_bwd_kernel_bit_for_bit(M, Cc, bf16, off):
    """g = (y == null || y > 0) ? dy : +0;  g_out = g;  dx = g * scale[c] (bf16: rounded to nearest even from the fp32 product), every
    combination of y / no y and g_out / no g_out; `off` = 1 moves every pointer by one element (the element-wise kernels).  y holds exact
    zeros and negative zeros (both mask), the scales both signs (a masked element times a negative scale is -0, as in the expression)."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    fn = lib.sd_frozen_bn_bwd_bf16 if bf16 else lib.sd_frozen_bn_bwd
    dt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator().manual_seed(M * 1000 + Cc)
    dy = torch.randn(M, Cc, generator=g).to(dt)
    y = torch.randn(M, Cc, generator=g).to(dt)
    flat = y.view(-1)
    flat[torch.randperm(flat.numel(), generator=g)[:max(flat.numel() // 7, 2)]] = 0.0
    flat[torch.randperm(flat.numel(), generator=g)[:max(flat.numel() // 9, 2)]] = -0.0
    assert (flat == 0).any() and (bits(flat) < 0).logical_and(flat == 0).any()
    scale = (torch.randn(Cc, generator=g) * 2).to(DEV)
    dyd, yd = _shifted(dy.to(DEV), off), _shifted(y.to(DEV), off)
    for with_y in (True, False):
        gm = torch.where(yd.float() > 0, dyd, torch.zeros_like(dyd)) if with_y else dyd
        want_dx = (gm.float() * scale).to(dt)
        for with_g in (True, False):
            outs = [torch.full((M * Cc + GUARD + off,), 3.0, dtype=dt, device=DEV) for _ in range(2)]
            dx, go = outs[0][off:off + M * Cc].view(M, Cc), outs[1][off:off + M * Cc].view(M, Cc)
            L.check(fn(dyd.data_ptr(), yd.data_ptr() if with_y else 0, scale.data_ptr(), M, Cc, dx.data_ptr(), go.data_ptr() if with_g else 0, L.stream()))
            torch.cuda.synchronize()
            assert torch.equal(bits(dx), bits(want_dx)), (with_y, with_g)
            if with_g:
                assert torch.equal(bits(go), bits(gm)), (with_y, with_g)
            else:
                assert (outs[1] == 3.0).all()
            for o in outs:                                  # nothing in front of or behind the M x C elements is written
                assert (o[:off] == 3.0).all() and (o[off + M * Cc:] == 3.0).all()
    # the launch the plan names for this call is the one that ran: vector kernels only with every pointer aligned (bf16: C % 8 == 0 holds here)
    text = lib.sd_nn_kernel_names(C.byref(L.NnCallDesc(op=25, form=int(bf16), M=M, C=Cc, flags=0 if off else 15))).decode()
    assert text.startswith("k_bn_frozen_bwd_ew<" if off else ("k_bn_frozen_bwd_bf16x8" if bf16 else "k_bn_frozen_bwd_f32x4")), text


# ---- the engine against the oracle ---------------------------------------------------------------------------------------------------------
def _args():
    return Namespace(labels={"l0": 0, "l1": 1}, parts={"p0": 0}, fpn_depth=128)


def _net(state):
    from structuredetector_amd.model import Network
    net = Network(_args(), pretrained=False, raw_output=True)
    net.load_state_dict(state)
    return net.to(DEV).train()


def _is_bn(m):
    return isinstance(m, torch.nn.BatchNorm2d)


def _frozen_bn_names(ref, N, bn):
    """state_dict prefixes of the oracle's BatchNorms that a freeze(N, bn) fixes"""
    names = []
    for k, stage in enumerate(STAGES):
        if k < N or bn:
            names += [f"{stage}.{n}" for n, m in getattr(ref, stage).named_modules() if _is_bn(m)]
    return names


def _freeze_oracle(ref, N, bn):
    """Detectron2's FREEZE_AT / FrozenBatchNorm2d on the oracle: the first N stages in eval mode without gradients; with `bn` the BatchNorms
    of the rest of the trunk in eval mode with fixed affine parameters."""
    ref.train()
    for k, stage in enumerate(STAGES):
        mod = getattr(ref, stage)
        if k < N:
            mod.eval()
            mod.requires_grad_(False)
        elif bn:
            for m in mod.modules():
                if _is_bn(m):
                    m.eval()
                    m.requires_grad_(False)
    return ref


@functools.lru_cache(maxsize=None)
def _case(B, H, W, N, bn, amp=False, seed=0):
    """One oracle run per case, shared: the state the nets start from (running statistics made sensible by one train-mode forward with
    momentum 1), input, output gradient, and the frozen oracle's output / gradients / buffers in fp32 (amp: under CPU autocast) and fp64."""
    g = torch.Generator().manual_seed(B * 100000 + H * 100 + W + seed)
    x = torch.randn(B, 3, H, W, generator=g)
    dy = torch.randn(B, 7, H // 4, W // 4, generator=g) * 0.1
    ref = O.build_reference_network(2, 1, seed=seed + 11)
    bns = [m for m in ref.modules() if _is_bn(m)]
    for m in bns:
        m.momentum = 1.0
    ref.train()
    with torch.no_grad():
        ref(torch.randn(B, 3, H, W, generator=g))
    for m in bns:
        m.momentum = 0.1
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    _freeze_oracle(ref, N, bn)
    ref64 = copy.deepcopy(ref).double()
    out64 = ref64(x.double())
    out64.backward(dy.double())
    if amp:
        with torch.autocast(device_type="cpu", dtype=torch.bfloat16):
            out32 = ref(x)
        out32.float().backward(dy)
    else:
        out32 = ref(x)
        out32.backward(dy)
    grads = lambda net: {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in net.named_parameters()}
    return dict(x=x, dy=dy, state=state, out32=out32.detach().float(), out64=out64.detach(), g32=grads(ref), g64=grads(ref64),
                buffers=dict(ref.named_buffers()), buffers64=dict(ref64.named_buffers()), frozen_bn=_frozen_bn_names(ref, N, bn))


def _run(case, N, bn, amp=False, junk=True):
    net = _net(case["state"])
    if junk:
        net.flat_grads.fill_(7.0)                           # `freeze` must zero the frozen slots; the backward overwrites the others
    net.freeze(N, bn)
    before = {k: v.clone() for k, v in net.named_buffers()}
    out, tape = net.forward_train(case["x"].to(DEV), amp=amp)
    net.backward_from(tape, case["dy"].to(DEV))
    torch.cuda.synchronize()
    return net, out, tape, before


def _check_frozen_state(net, case, before, N, bn, tol=1e-5):
    """frozen slots of the gradient exactly zero; frozen BatchNorm buffers bit-identical and not counted; the others as the oracle's"""
    params = dict(net.named_parameters())
    trainable = [n for n, g in case["g64"].items() if g is not None]
    assert {n for n, p in params.items() if p.requires_grad} == set(trainable)
    lo, off = net.frozen_range()
    assert lo == 0 and off == (min(net._flat_off[id(params[n])][0] for n in params if n.split(".")[0] not in STAGES[:N]))
    assert not net.flat_grads[:off].any()
    for n, p in params.items():
        if n not in trainable:
            assert not net.grad_of(p).any(), n
    for name, b in net.named_buffers():
        frozen = name.rsplit(".", 1)[0] in case["frozen_bn"]
        if frozen:
            assert torch.equal(b, before[name]), name
        elif b.dtype == torch.long:
            assert int(b) == int(before[name]) + 1 == int(case["buffers"][name]), name
        elif tol is not None:
            close(b.cpu(), case["buffers"][name], tol)
            assert not torch.equal(b, before[name]), name
    return trainable


@pytest.mark.parametrize("N", [1, 2, 3, 5])
@pytest.mark.parametrize("B,H,W", [(3, 64, 96), (2, 64, 64)])
def test_frozen_stages_output_and_gradients_vs_oracle(B, H, W, N):
    case = _case(B, H, W, N, False)
    net, out, tape, before = _run(case, N, False)
    assert len(tape["blocks"]) == sum(n for k, n in enumerate((3, 4, 6, 3), start=1) if k >= N) and tape["stem"] is None
    close(out.cpu(), case["out32"], 1e-4)
    trainable = _check_frozen_state(net, case, before, N, False)
    params = dict(net.named_parameters())
    gpu = torch.cat([net.grad_of(params[n]).cpu().double().flatten() for n in trainable])
    cpu = torch.cat([case["g32"][n].double().flatten() for n in trainable])
    tru = torch.cat([case["g64"][n].flatten() for n in trainable])
    e_gpu, e_cpu = float((gpu - tru).norm() / tru.norm()), float((cpu - tru).norm() / tru.norm())
    print(f"B={B} {H}x{W} N={N}: gradient vs fp64 oracle {e_gpu:.3e} (fp32 oracle {e_cpu:.3e})")
    assert e_gpu <= 3e-2, (e_gpu, e_cpu)
    for n in ("head.conv.weight", "head.conv.bias"):
        close(net.grad_of(params[n]).cpu().double(), case["g64"][n], 1e-5)


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("B,H,W", [(3, 64, 96), (2, 64, 64)])
def test_frozen_batchnorm_in_the_trainable_trunk_vs_oracle(B, H, W, N):
    from structuredetector_amd.model.network import FrozenBnRec
    case = _case(B, H, W, N, True)
    net, out, tape, before = _run(case, N, True)
    assert tape["blocks"] and all(isinstance(b, FrozenBnRec) for b in tape["blocks"])
    close(out.cpu(), case["out32"], 1e-4)
    trainable = _check_frozen_state(net, case, before, N, True)
    assert not any(n.startswith("down") and (".bn" in n or ".downsample.1." in n) for n in trainable)
    # no trunk running statistic changed; the FPN's (batch statistics, as before) did
    for name, b in net.named_buffers():
        assert torch.equal(b, before[name]) == name.startswith(("adpater", "down")), name
    params = dict(net.named_parameters())
    gpu = torch.cat([net.grad_of(params[n]).cpu().double().flatten() for n in trainable])
    cpu = torch.cat([case["g32"][n].double().flatten() for n in trainable])
    tru = torch.cat([case["g64"][n].flatten() for n in trainable])
    e_gpu, e_cpu = float((gpu - tru).norm() / tru.norm()), float((cpu - tru).norm() / tru.norm())
    print(f"B={B} {H}x{W} N={N} frozen BN: gradient vs fp64 oracle {e_gpu:.3e} (fp32 oracle {e_cpu:.3e})")
    assert e_gpu <= 3e-2, (e_gpu, e_cpu)
    for n in ("head.conv.weight", "head.conv.bias"):
        close(net.grad_of(params[n]).cpu().double(), case["g64"][n], 1e-5)


@pytest.mark.parametrize("bn", [False, True], ids=["stages", "stages+bn"])
def test_mixed_precision_frozen_step_vs_autocast_oracle(bn):
    """N = 2 under `--amp`, by the error populations of tests/test_gpu_amp.py: as close to an fp64 run of the frozen oracle as the frozen
    oracle under CPU autocast is (median, mean and maximum over the trainable parameter tensors, that file's margins)."""
    case = _case(8, 128, 128, 2, bn, amp=True)
    net, out, tape, before = _run(case, 2, bn, amp=True)
    assert out.dtype == torch.float32 and tape["amp"] is True and tape["f1"].dtype == torch.bfloat16
    trainable = _check_frozen_state(net, case, before, 2, bn, tol=None)
    scale = case["out64"].abs().max().item()
    e_fwd_gpu = (out.cpu().double() - case["out64"]).abs().max().item() / scale
    e_fwd_ac = (case["out32"].double() - case["out64"]).abs().max().item() / scale
    assert e_fwd_gpu <= 2 * e_fwd_ac + 1e-3, (e_fwd_gpu, e_fwd_ac)
    params = dict(net.named_parameters())
    e_gpu, e_ac = [], []
    for n in trainable:
        truth = case["g64"][n]
        s = truth.abs().max().item() + 1e-30
        e_gpu.append((net.grad_of(params[n]).cpu().double() - truth).abs().max().item() / s)
        e_ac.append((case["g32"][n].double() - truth).abs().max().item() / s)
    e_gpu, e_ac = np.array(e_gpu), np.array(e_ac)
    print(f"amp N=2 bn={bn}: forward {e_fwd_gpu:.3e} (autocast {e_fwd_ac:.3e}); gradients median {np.median(e_gpu):.3e} ({np.median(e_ac):.3e}) "
          f"mean {np.mean(e_gpu):.3e} ({np.mean(e_ac):.3e}) max {e_gpu.max():.3e} ({e_ac.max():.3e})")
    assert np.isfinite(e_gpu).all()
    assert np.median(e_gpu) <= 2 * np.median(e_ac) + 1e-3, (np.median(e_gpu), np.median(e_ac))
    assert np.mean(e_gpu) <= 2 * np.mean(e_ac) + 1e-3, (np.mean(e_gpu), np.mean(e_ac))
    assert e_gpu.max() <= 2 * e_ac.max() + 1e-2, (e_gpu.max(), e_ac.max())
    # the running statistics of the BatchNorms that still train, as close to the fp64 run's as the autocast oracle's are
    eb_gpu, eb_ac = [], []
    for name, b in net.named_buffers():
        if b.dtype == torch.long or name.rsplit(".", 1)[0] in case["frozen_bn"]:
            continue
        s = case["buffers64"][name].abs().max().item() + 1e-30
        eb_gpu.append((b.cpu().double() - case["buffers64"][name]).abs().max().item() / s)
        eb_ac.append((case["buffers"][name].double() - case["buffers64"][name]).abs().max().item() / s)
    assert np.median(eb_gpu) <= 2 * np.median(eb_ac) + 1e-3 and max(eb_gpu) <= 2 * max(eb_ac) + 1e-2, (np.median(eb_gpu), np.median(eb_ac), max(eb_gpu), max(eb_ac))


def test_autograd_path_gives_the_same_gradients_and_none_for_frozen_parameters():
    case = _case(2, 64, 64, 2, True)
    net, _, _, _ = _run(case, 2, True, junk=False)
    net2 = _net(case["state"]).freeze(2, True)
    out = net2(case["x"].to(DEV))
    out.backward(case["dy"].to(DEV))
    assert torch.equal(net2.flat_grads, net.flat_grads)
    for n, p in net2.named_parameters():
        assert (p.grad is None) == (case["g64"][n] is None), n
        if p.grad is not None:
            assert torch.equal(p.grad, net2.grad_of(p)), n


def test_freeze_zero_is_the_network_that_was_never_frozen():
    case = _case(2, 64, 64, 1, False)
    x, dy = case["x"].to(DEV), case["dy"].to(DEV)
    res = []
    for thaw in (False, True):
        net = _net(case["state"])
        if thaw:
            net.freeze(3, True).freeze(0, False)
        out, tape = net.forward_train(x)
        net.backward_from(tape, dy)
        res.append((out.clone(), net.flat_grads.clone(), [b.clone() for b in net.buffers()]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
    assert all(p.requires_grad for p in net.parameters()) and net.frozen_range() == (0, 0)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_refreezing_after_thawed_steps_reads_the_trained_weights(amp):
    """freeze -> step -> freeze(0) -> steps that train the trunk -> freeze again, no train() call between: the re-frozen layers run on the
    weights and BatchNorm statistics as they are NOW (their cached folds and bf16 copies are dropped by `freeze`), bit for bit what a
    network that loads the same state and is frozen once computes."""
    _, net, step, batches = _step_setup(stages=2, bn=True)
    step.amp = amp
    step(*batches[0])                                       # fills the caches of the frozen layers
    net.freeze(0)
    from structuredetector_amd.model.trainer import TrainStep
    thawed = TrainStep(net, step.args)
    thawed.amp = amp
    before = net.flat_params.clone()
    for k in range(2):
        thawed(*batches[k % 2])
    off = net.freeze(2, True).frozen_range()[1]
    assert not torch.equal(net.flat_params[:off], before[:off])           # the stages that are frozen again did train
    x = batches[0][0]
    out, _ = net.forward_train(x, amp=amp)
    _, fresh, _, _ = _step_setup(stages=0, bn=False)
    fresh.load_state_dict(net.state_dict())
    fresh.freeze(2, True)
    want, _ = fresh.forward_train(x, amp=amp)
    assert torch.equal(out, want)


def test_freeze_survives_the_move_to_the_device():
    from structuredetector_amd.model import Network
    case = _case(2, 64, 64, 2, True)
    net = Network(_args(), pretrained=False, raw_output=True)
    net.load_state_dict(case["state"])
    net.freeze(2, True)                                     # before .to(device)
    net = net.to(DEV).train()
    assert (net.frozen_stages, net.frozen_bn) == (2, True)
    ref, _, _, _ = _run(case, 2, True, junk=False)
    out, tape = net.forward_train(case["x"].to(DEV))
    net.backward_from(tape, case["dy"].to(DEV))
    assert torch.equal(net.flat_grads, ref.flat_grads) and not net.flat_grads[:net.frozen_range()[1]].any()


def test_refusals():
    from structuredetector_amd import _lib as L
    case = _case(2, 64, 64, 1, False)
    net = _net(case["state"])
    with pytest.raises(ValueError, match="stages >= 1"):
        net.freeze(0, bn=True)
    with pytest.raises(ValueError):
        net.freeze(6)
    net.freeze(1)
    net._engine.fuse_bn_bwd = True
    with pytest.raises(L.SdError, match="fuse_bn_bwd"):
        net.forward_train(case["x"].to(DEV))
    net._engine.fuse_bn_bwd = False
    out, tape = net.forward_train(case["x"].to(DEV))
    net._engine.fuse_bn_bwd = True
    with pytest.raises(L.SdError, match="fuse_bn_bwd"):
        net.backward_from(tape, case["dy"].to(DEV))


# ---- the step --------------------------------------------------------------------------------------------------------------------------------
OPTIONS = dict(weight_decay=0.05, clip_grad_norm=0.5, ema_decay=0.9)


def _step_setup(seed=9, stages=2, bn=True, **kw):
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    from tests.test_host_cpu import make_args
    dev = torch.device("cuda", 0)
    args = make_args(2, 1, 20, 40, device=dev, learning_rate=1e-3)
    torch.manual_seed(seed)
    net = Network(args, pretrained=False).to(dev).train()
    with torch.no_grad():                                   # BatchNorm affines and statistics that are not the identity
        g = torch.Generator().manual_seed(seed)
        for m in net.modules():
            if hasattr(m, "running_var"):
                m.weight.copy_(1 + 0.1 * torch.randn(m.c, generator=g)); m.bias.copy_(0.1 * torch.randn(m.c, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.c, generator=g)); m.running_var.copy_(1 + 0.2 * torch.rand(m.c, generator=g))
    net.freeze(stages, bn)
    enc = Encode(args)
    batches = []
    for k in range(2):
        tgt = enc.render(enc.plan(128, 128, *synthetic_batch(np.random.default_rng(100 + k), 2, 128, 128, 2, 1)), dev)
        x = torch.randn(2, 3, 128, 128, device=dev, generator=torch.Generator(dev).manual_seed(200 + k))
        batches.append((x, tgt))
    return args, net, TrainStep(net, args, **kw), batches


def test_four_steps_leave_everything_frozen_bit_identical_and_resume_continues():
    from structuredetector_amd.model.network import BNParams
    args, net, step, batches = _step_setup(**OPTIONS)
    assert step.frozen == (2, True) and step.frozen_off == net.frozen_range()[1] > 0
    off = step.frozen_off
    p0, ema0 = net.flat_params.clone(), step.ema.clone()
    buffers0 = {k: v.clone() for k, v in net.named_buffers()}
    for k in range(4):
        step(*batches[k % 2])
    torch.cuda.synchronize()
    assert int(step.skipped_steps) == 0 and float(step.grad_norm) > 0
    assert torch.equal(net.flat_params[:off], p0[:off]) and torch.equal(step.ema[:off], ema0[:off])
    assert not step.exp_avg[:off].any() and not step.exp_avg_sq[:off].any() and not net.flat_grads[:off].any()
    fixed = changed = 0
    for name, m in net.named_modules():
        if isinstance(m, BNParams) and name.startswith("down"):          # every trunk BatchNorm: in the prefix or frozen inside the suffix
            for p in (m.weight, m.bias):
                o, n = net._flat_off[id(p)]
                assert torch.equal(net.flat_params[o:o + n], p0[o:o + n]), name
                assert not step.exp_avg[o:o + n].any() and not step.exp_avg_sq[o:o + n].any(), name
                fixed += o >= off
    assert fixed == 2 * (9 + 13 + 7)                                     # down2 .. down4: two per block plus the three downsample ones
    for name, p in net.named_parameters():
        if p.requires_grad:
            o, n = net._flat_off[id(p)]
            assert not torch.equal(net.flat_params[o:o + n], p0[o:o + n]), name
            changed += 1
    assert changed > 0 and not torch.equal(step.ema[off:], ema0[off:])
    for name, b in net.named_buffers():
        assert torch.equal(b, buffers0[name]) == name.startswith(("adpater", "down")), name
    # deterministic over two runs
    _, net_b, step_b, _ = _step_setup(**OPTIONS)
    for k in range(4):
        step_b(*batches[k % 2])
    assert torch.equal(net_b.flat_params, net.flat_params) and torch.equal(step_b.ema, step.ema)
    # two steps, state_dict -> load_state_dict into a fresh step (whose moments the load refills), two more steps
    _, net_c, step_c, _ = _step_setup(**OPTIONS)
    for k in range(2):
        step_c(*batches[k % 2])
    state = {"model": {k: v.detach().cpu().clone() for k, v in net_c.state_dict().items()}, "optimizer": step_c.state_dict()}
    state["optimizer"]["exp_avg"][:off] = 1.0                             # a state from a run that trained these slots: the load zeroes them
    _, net_d, step_d, _ = _step_setup()
    net_d.load_state_dict(state["model"])
    step_d.load_state_dict(state["optimizer"])
    assert not step_d.exp_avg[:off].any()
    for k in range(2, 4):
        step_d(*batches[k % 2])
    torch.cuda.synchronize()
    assert torch.equal(net_d.flat_params, net.flat_params) and torch.equal(step_d.ema, step.ema)
    assert torch.equal(step_d.exp_avg, step.exp_avg) and torch.equal(step_d.exp_avg_sq, step.exp_avg_sq)


def test_sync_bn_at_world_one_gives_the_same_bits_and_logs_unfrozen_batchnorms_only():
    _, net_a, step_a, batches = _step_setup(bn=False)
    _, net_b, step_b, _ = _step_setup(bn=False, sync_bn=True)
    step_b.bn_sync.log = []
    for k in range(2):
        la, lb = step_a(*batches[k % 2]), step_b(*batches[k % 2])
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    assert torch.equal(net_a.flat_params, net_b.flat_params)
    assert all(torch.equal(a, b) for a, b in zip(net_a.buffers(), net_b.buffers()))
    # 39 BatchNorms, 7 of them in the stem and down1: one entry per remaining BatchNorm and direction
    assert len(step_b.bn_sync.log) == 2 * 2 * (39 - 7), len(step_b.bn_sync.log)
    assert not any("stem" in name or "maxpool" in name for name in step_b.bn_sync.log)
    # frozen BatchNorm as well: only the FPN's three are left
    _, net_c, step_c, _ = _step_setup(bn=True, sync_bn=True)
    step_c.bn_sync.log = []
    step_c(*batches[0])
    assert len(step_c.bn_sync.log) == 2 * 3, step_c.bn_sync.log
