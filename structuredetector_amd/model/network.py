"""`Network`: ResNet-34 trunk + 3-level FPN + 1x1 head on hand-written HIP kernels.

Mirrors `Network` / `Fpn` / `Head` of src/sdnet/model/network.py:6-87 and the torchvision
resnet34 pieces it borrows (conv1/bn1/relu/maxpool/layer1-4; BasicBlock [3,4,6,3]):
same constructor signature, same `forward(x) -> dict` of four channel-slice views (or the raw
tensor with `raw_output=True`), same `save()`, and the same state_dict key schema (including the
`adpater` spelling) so reference `.pth` checkpoints load unchanged.

Mechanism (MI355X-first, not a module-by-module translation):
  * every learnable tensor lives in ONE flat fp32 device buffer (`flat_params`), gradients in a
    second one (`flat_grads`): the optimizer is a single fused Adam launch and the data-parallel
    exchange is a single RCCL all-reduce over the flat gradient buffer;
  * activations are NHWC, conv weights [Cout][R][S][Cin] (the parameters are exposed with OIHW
    *logical* shape and channels_last strides, so state_dicts stay interchangeable);
  * forward and backward are explicit kernel schedules (`_Engine`) behind one autograd node;
    no torch.nn.functional / MIOpen call is made anywhere.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from typing import NamedTuple

import torch
import torch.nn as nn

from .. import _lib as L
from ..utils import trace as T

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
FREEZE_STAGES = ("adpater", "down1", "down2", "down3", "down4")     # `Network.freeze(stages=N)`: the first N, in the order of parameters()
OPTIM_STAGES = FREEZE_STAGES + ("fpn", "head")                      # `Network.optim_groups()`: the trunk, then up1 .. up4, then the head


# ------------------------------------------------------------------------------------------
# parameter containers (no compute): they only give the state_dict its reference key names
# ------------------------------------------------------------------------------------------
class ConvParams(nn.Module):
    def __init__(self, cin, cout, k, stride=1, pad=0, bias=False):
        super().__init__()
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, k, stride, pad
        w = torch.empty((cout, cin, k, k), memory_format=torch.channels_last)
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None


class BNParams(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.c = c
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class Slot(nn.Module):
    """Parameter-less position (ReLU / MaxPool / Upsample) kept so Sequential indices match the reference."""


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = ConvParams(cin, cout, 3, stride, 1)
        self.bn1 = BNParams(cout)
        self.relu = Slot()
        self.conv2 = ConvParams(cout, cout, 3, 1, 1)
        self.bn2 = BNParams(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(ConvParams(cin, cout, 1, stride, 0), BNParams(cout))


class Fpn(nn.Module):
    """network.py:6-19: conv3x3+BN+ReLU( upsample2x(input) + lateral1x1(shortcut) )."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.up = Slot()
        self.lateral = ConvParams(in_channels, out_channels, 1, bias=True)
        self.conv = nn.Sequential(ConvParams(out_channels, out_channels, 3, 1, 1), BNParams(out_channels), Slot())


class Head(nn.Module):
    """network.py:22-29."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = ConvParams(in_channels, out_channels, 1, bias=True)


BACKBONE_FILE_GLOB = "resnet34-*.pth"          # torchvision ResNet34_Weights.DEFAULT = IMAGENET1K_V1 = resnet34-b627a593.pth


def find_backbone_weights(args=None):
    """Local lookup of the ImageNet ResNet-34 checkpoint `pretrained=True` asks for (network.py:41), in this order:
    `args.backbone_weights`, $SDNET_BACKBONE_WEIGHTS (both must exist when given), then `resnet34-*.pth` in the directories
    torchvision / torch.hub would have cached it in ($TORCH_HOME/hub/checkpoints, $XDG_CACHE_HOME/torch/hub/checkpoints,
    ~/.cache/torch/hub/checkpoints).  Returns a Path or None; never downloads."""
    import os
    from pathlib import Path
    for given in (getattr(args, "backbone_weights", None), os.environ.get("SDNET_BACKBONE_WEIGHTS")):
        if given:
            path = Path(given).expanduser()
            if not path.is_file():
                raise L.SdError(f"backbone weights file not found: {path}")
            return path
    homes = []
    if os.environ.get("TORCH_HOME"):
        homes.append(Path(os.environ["TORCH_HOME"]))
    homes.append(Path(os.environ.get("XDG_CACHE_HOME", "~/.cache")).expanduser() / "torch")
    for home in homes:
        hits = sorted((home / "hub" / "checkpoints").glob(BACKBONE_FILE_GLOB))
        if hits:
            return hits[0]
    return None


def _layer(cin, cout, n, stride):
    return nn.Sequential(*[BasicBlock(cin if i == 0 else cout, cout, stride if i == 0 else 1) for i in range(n)])


# ------------------------------------------------------------------------------------------
# kernel schedule
# ------------------------------------------------------------------------------------------
def _desc(B, Hi, Wi, conv: ConvParams):
    d = L.ConvDesc()
    d.B, d.Hi, d.Wi, d.Cin, d.Cout, d.R, d.S, d.stride, d.pad = B, Hi, Wi, conv.cin, conv.cout, conv.k, conv.k, conv.stride, conv.pad
    d.Ho = (Hi + 2 * conv.pad - conv.k) // conv.stride + 1
    d.Wo = (Wi + 2 * conv.pad - conv.k) // conv.stride + 1
    return d


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _flops(d):
    return 2.0 * d.B * d.Ho * d.Wo * d.Cout * d.Cin * d.R * d.S


# ReLU-mask mode of the BatchNorm backward kernels: no ReLU / mask from the saved output y / mask recomputed from x / y holds the
# mask bytes of sd_bn_apply (residual layers)
RELU_NONE, RELU_FROM_Y, RELU_FROM_X, RELU_MASK_BYTES = 0, 1, 2, 3


def _mask_ptr(y, relu):
    """the `y` pointer a ReLU-mask mode reads (the other two modes take none)"""
    return _ptr(y) if relu in (RELU_FROM_Y, RELU_MASK_BYTES) else 0


# what the training forward leaves on the tape for the backward; positional order is part of the contract (tests unpack them)
class StemRec(NamedTuple):
    d: object; s0: object; mean: object; invstd: object; pidx: object


class BlockRec(NamedTuple):
    blk: object; xin: object; hw: tuple; d1: object; c1: object; a1: object; m1: object; i1: object; d2: object; c2: object; m2: object
    i2: object; out: object; dd: object; cd: object; md: object; idd: object; mask: object


class FrozenBnRec(NamedTuple):
    """a trainable block whose BatchNorms are frozen (`Network.freeze(bn=True)`): the eval schedule's three launches, no statistics;
    scales = the folded (conv1, conv2, downsample or None) BatchNorm scales its backward multiplies by"""
    blk: object; xin: object; hw: tuple; d1: object; a1: object; d2: object; out: object; dd: object; idt: object; scales: tuple


class FpnRec(NamedTuple):
    fpn: object; shortcut: object; hw: tuple; dl: object; t: object; dc: object; c: object; mean: object; invstd: object; out: object


class LateralGrad(NamedTuple):
    """deferred data-gradient of an FPN lateral 1x1: joins the trunk's own gradient of the same tensor"""
    dy: object; conv: object; d: object


class _Engine:
    """Explicit forward / backward schedules over the C ABI.  Tensors named *_nhwc are
    (B, H, W, C) contiguous; `tape` keeps what the backward needs (StemRec, BlockRec and FpnRec records)."""

    def __init__(self, net: "Network"):
        self.net = net
        self.lib = L.lib()
        self.prof = None      # list -> every conv launch appends (kernel, algorithmic flops, start event, end event, phase)
        self.prof_shapes = None   # list -> the geometry of every labelled launch, in the order of `prof` (tools/step_layers.py)
        self._nbt = []        # num_batches_tracked counters touched by the running forward (bumped with one launch)
        # Optional: weight-gradient GEMMs on a side stream (they only depend on the layer's output gradient), free-running
        # beside the data-gradient chain.  Measured +3.5 % images/s at bs=64 in round 3 and -3 % in round 4 (the row-ring weight gradient's
        # 512-thread block owns 152 KB of LDS: no conv block fits beside it); OFF by default because concurrent kernels
        # stretch each other's durations and the per-kernel roofline numbers of bench.py / rocprofv3 stop describing a
        # kernel running alone.  (Chaining dgrad -> wgrad -> dgrad across the streams so that only the BatchNorm passes
        # overlap was measured too: slower than no overlap, the HBM-bound passes slow the wgrad they run under.)
        self.overlap_wgrad = False
        self._side = None
        # BatchNorm-backward reduction inside the data-gradient epilogue (sd_conv2d_dgrad_bn_reduce).  Measured at bs=64: with the
        # first (4-byte) epilogue it cost the conv kernels 4.0 ms to save 2.2 ms of reduce passes; with the 16-byte epilogue
        # (float4 reads of the BatchNorm input, mask bytes) it is exactly neutral (815.7 vs 815.4 img/s): the reduce passes it
        # removes run at HBM speed anyway.  Off by default; the path is kept and tested (tests/test_gpu_network.py).
        self.fuse_bn_bwd = False
        self._wt_plan, self._wt_flat, self._wt_valid = None, {}, None      # transposed data-gradient weights (see _transpose_all)
        self._head_ok = {}
        self.stem_ring = True              # mixed-precision step: bf16 stem gradient + the row-ring stem weight gradient (False: fp32 gradient + k_stem_wgrad_bf16; A/B)
        self.fuse_head = True              # bf16 inference: the 1x1 head in the epilogue of the last FPN conv where it takes the two-group kernel (False: A/B, tests)
        self.small_batch_kernel = True     # eval forward: sd_conv2d_fwd_sb where the 128-row tile grid cannot fill the chip (False: A/B)

    def _tic(self, d, which, bf16=False, name=None):
        """Opens the `prof` record of a conv launch (None while `prof` is off).  The label is the device kernel the C ABI will launch
        for pass `which` of this conv (same names as the rocprofv3 kernel trace), or `name` where the caller knows it."""
        if self.prof is None:
            return None
        if name is None:
            if self.prof_shapes is not None:
                self.prof_shapes.append((d.B, d.Hi, d.Wi, d.Cin, d.Cout, d.R, d.stride, d.Ho, d.Wo))
            name = self.lib.sd_conv2d_kernel_name(C.byref(d), which).decode()
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()           # torch's current stream == the stream handed to the C ABI (L.stream())
        return ("bf16:" + name if bf16 else name), e0

    def _toc(self, t, d, phase="fwd"):
        if t is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.prof.append((t[0], _flops(d), t[1], e1, phase))

    # ---- helpers -------------------------------------------------------------------------
    def _ws(self, nbytes, dev):
        return L.workspace(max(int(nbytes), 256), dev)

    def _fn(self, name, bf16):
        """the fp32 / bf16 pair of an entry point: the bf16 one carries the suffix"""
        return getattr(self.lib, name + "_bf16" if bf16 else name)

    @staticmethod
    def _running(bn, update):
        """running-statistics pointer pair of a statistics launch (0, 0: leave them alone)"""
        return (bn.running_mean.data_ptr(), bn.running_var.data_ptr()) if update else (0, 0)

    @staticmethod
    def _w32(conv):
        return conv.weight

    # ---- mixed precision (`--amp`, trainer.py:115-121): bf16 activations / conv weights, fp32 accumulation and master weights ----
    def _to_bf16(self, t):
        out = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
        L.check(self.lib.sd_cast_f32_to_bf16(t.data_ptr(), out.data_ptr(), t.numel(), L.stream()), "sd_cast_f32_to_bf16")
        return out

    def _to_f32(self, t):
        out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
        L.check(self.lib.sd_cast_bf16_to_f32(t.data_ptr(), out.data_ptr(), t.numel(), L.stream()), "sd_cast_bf16_to_f32")
        return out

    def refresh_bf16_weights(self):
        """One cast of the whole flat fp32 parameter buffer per step; every conv weight is then a view at its fp32 offset."""
        net = self.net
        if net.flat_params_bf16 is None:
            net.flat_params_bf16 = torch.empty(net.flat_params.numel(), dtype=torch.bfloat16, device=net.flat_params.device)
        L.check(self.lib.sd_cast_f32_to_bf16(net.flat_params.data_ptr(), net.flat_params_bf16.data_ptr(), net.flat_params.numel(), L.stream()),
                "sd_cast_f32_to_bf16")

    def _w16(self, conv):
        off, n = self.net._flat_off[id(conv.weight)]
        return self.net.flat_params_bf16[off:off + n]                 # physical [Cout][R][S][Cin] order; off % 8 == 0 (32-byte slots): 16-byte aligned

    def conv(self, how, x, conv, B, Hi, Wi, scale=None, shift=None, res=None, res_up2=False, relu=False):
        """The conv forward launch of every schedule.  how = (weight source, entry point, its workspace query or None: no split-K
        workspace, kernel-name pass 0 = fp32 / 16 = bf16, try the small-batch kernel first, give the launch a `prof` record).
        Small-batch kernel (sd_conv2d_fwd_sb): one launch, split-K combined inside it; the arrival tickets live in a zeroed per-stream
        state buffer that every launch leaves zero."""
        weight, fwd, ws_bytes, which, sb, timed = how
        lib, bf16 = self.lib, int(which == 16)
        d = _desc(B, Hi, Wi, conv)
        y = torch.empty((B, d.Ho, d.Wo, conv.cout), dtype=torch.bfloat16 if bf16 else torch.float32, device=x.device)
        if sb and self.small_batch_kernel and lib.sd_conv2d_fwd_sb_supported(C.byref(d), bf16):
            w = weight(conv)
            nws = lib.sd_conv2d_fwd_sb_workspace_bytes(C.byref(d), bf16)
            ws = self._ws(nws, x.device) if nws else None
            st = L.zero_state(lib.sd_conv2d_fwd_sb_state_bytes(C.byref(d), bf16), x.device) if nws else None
            t = self._tic(d, which, name="k_conv_fwd_sb<false>") if timed else None          # (only fp32 schedules are timed)
            L.check(lib.sd_conv2d_fwd_sb(x.data_ptr(), w.data_ptr(), y.data_ptr(), C.byref(d), _ptr(scale), _ptr(shift), _ptr(res), int(res_up2),
                                         int(relu), bf16, _ptr(ws), ws.numel() if nws else 0, _ptr(st), st.numel() if nws else 0, L.stream()),
                    "sd_conv2d_fwd_sb")
        else:
            nws = ws_bytes(C.byref(d)) if ws_bytes is not None else 0          # > 0 only for small batches (split-K)
            ws = self._ws(nws, x.device) if nws else None
            w = weight(conv)
            t = self._tic(d, which, bf16) if timed else None
            L.check(fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), C.byref(d), _ptr(scale), _ptr(shift), _ptr(res), int(res_up2), int(relu),
                        _ptr(ws), ws.numel() if nws else 0, L.stream()), "sd_conv2d_fwd")
        if t is not None:
            self._toc(t, d)
        return y, d

    def conv_stats(self, x, conv, B, Hi, Wi, bn: BNParams, update_running=True, amp=False, sync=None):
        """Training forward of conv -> BatchNorm: the conv launch also produces the batch statistics of its output
        (sd_conv2d_fwd_bn_stats), so bn_train(..., stats=...) only has the apply pass left.  `sync` (a BnStatsExchange): the same
        launch stops after the first half of the statistics finish, the fp64 sums are exchanged, the second half finishes."""
        lib = self.lib
        d = _desc(B, Hi, Wi, conv)
        y = torch.empty((B, d.Ho, d.Wo, conv.cout), dtype=torch.bfloat16 if amp else torch.float32, device=x.device)
        mean = torch.empty(conv.cout, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        if sync is not None:
            sums = sync.take(conv.cout)
            if sync.log is not None:
                fused = lib.sd_conv2d_fwd_bn_stats_rows(C.byref(d), int(amp)) > 0
                sync.log.append(("sd_conv2d_fwd_bf16_bn_sums" if amp else "sd_conv2d_fwd_bn_sums") + ("" if fused else ":two-pass"))
            tail = (sums.data_ptr(),)
        else:
            tail = (BN_EPS, BN_MOMENTUM, *self._running(bn, update_running), mean.data_ptr(), invstd.data_ptr())
        if amp:
            fwd = lib.sd_conv2d_fwd_bf16_bn_stats if sync is None else lib.sd_conv2d_fwd_bf16_bn_sums
            w, ws_bytes = self._w16(conv), lib.sd_conv2d_fwd_bf16_bn_stats_workspace_bytes
        else:
            fwd = lib.sd_conv2d_fwd_bn_stats if sync is None else lib.sd_conv2d_fwd_bn_sums
            w, ws_bytes = conv.weight, lib.sd_conv2d_fwd_bn_stats_workspace_bytes
        ws = self._ws(ws_bytes(C.byref(d)), x.device)
        t = self._tic(d, 16 if amp else 0, amp)
        L.check(fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), C.byref(d), *tail, ws.data_ptr(), ws.numel(), L.stream()), "sd_conv2d_fwd_bn_stats")
        self._toc(t, d)
        if sync is not None:
            self._stats_from_sums(sync, sums, bn, mean, invstd, update_running)
        return y, d, (mean, invstd)

    def _stats_from_sums(self, sync, sums, bn: BNParams, mean, invstd, update_running=True):
        """Synchronized BatchNorm, forward: all-reduce the layer's fp64 [S0, S1, n], then mean / invstd / running statistics from it."""
        sync.reduce(sums)
        L.check(self.lib.sd_bn_stats_from_sums(sums.data_ptr(), bn.c, BN_EPS, BN_MOMENTUM, *self._running(bn, update_running),
                                               mean.data_ptr(), invstd.data_ptr(), L.stream()), "sd_bn_stats_from_sums")

    def _means_from_sums(self, sync, sums, Cc, device):
        """Synchronized BatchNorm, backward: all-reduce [sum g, sum g * xhat, n], then the two per-channel means of the apply pass."""
        sync.reduce(sums)
        means = torch.empty(2 * Cc, dtype=torch.float32, device=device)
        L.check(self.lib.sd_bn_bwd_means_from_sums(sums.data_ptr(), Cc, means.data_ptr(), L.stream()), "sd_bn_bwd_means_from_sums")
        return means

    def bn_train(self, x, bn: BNParams, res=None, relu=True, update_running=True, stats=None, want_mask=False, sync=None):
        Mrows, Cc = x.numel() // x.shape[-1], x.shape[-1]
        bf16 = x.dtype == torch.bfloat16
        if stats is not None:
            mean, invstd = stats
        else:
            mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
            invstd = torch.empty_like(mean)
            ws = self._ws(self.lib.sd_col_reduce_workspace_bytes(Mrows, Cc), x.device)
            if sync is not None:
                sums = sync.take(Cc)
                sync.record("sd_bn_train_sums")
                L.check(self._fn("sd_bn_train_sums", bf16)(x.data_ptr(), Mrows, Cc, sums.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()),
                        "sd_bn_train_sums")
                self._stats_from_sums(sync, sums, bn, mean, invstd, update_running)
            else:
                L.check(self.lib.sd_bn_train_stats(x.data_ptr(), Mrows, Cc, BN_EPS, BN_MOMENTUM, *self._running(bn, update_running),
                                                   mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "sd_bn_train_stats")
        y = torch.empty_like(x)
        # residual layers: the backward needs the ReLU mask of y; one byte per four elements instead of re-reading y twice
        mask = torch.empty(x.numel() // 4, dtype=torch.uint8, device=x.device) if want_mask else None
        L.check(self._fn("sd_bn_apply", bf16)(x.data_ptr(), y.data_ptr(), Mrows, Cc, mean.data_ptr(), invstd.data_ptr(), bn.weight.data_ptr(),
                                              bn.bias.data_ptr(), _ptr(res), int(relu), _ptr(mask), L.stream()), "sd_bn_apply")
        if update_running:
            self._nbt.append(bn.num_batches_tracked)
        return (y, mean, invstd, mask) if want_mask else (y, mean, invstd)

    def bn_fold(self, bn: BNParams):
        cached = self.net._folded.get(id(bn))
        if cached is not None:
            return cached
        scale = torch.empty(bn.c, dtype=torch.float32, device=bn.weight.device)
        shift = torch.empty_like(scale)
        L.check(self.lib.sd_bn_fold(bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                    BN_EPS, bn.c, scale.data_ptr(), shift.data_ptr(), L.stream()), "sd_bn_fold")
        self.net._folded[id(bn)] = (scale, shift)
        return scale, shift

    # ---- forward -------------------------------------------------------------------------
    @staticmethod
    def _input(x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise L.SdError(f"Network expects (B, 3, H, W) input, got {tuple(x.shape)}")
        L.require_cuda(x)
        x = x.contiguous().float()
        B, _, H, W = x.shape
        if H % 32 or W % 32:
            raise L.SdError("input height/width must be multiples of 32 (args.py:181-186)")
        return x, B, H, W

    def forward(self, x, training, tape=None, amp=False):
        """training=False: the fp32 eval schedule (_eval).  training=True: the training forward, recording `tape` for backward();
        amp: the mixed-precision step."""
        if not training:
            if amp:
                raise L.SdError("amp=True is the mixed-precision TRAINING forward; inference uses forward_bf16")
            return self._eval(x, False)
        net, lib = self.net, self.lib
        nf, fbn = net.frozen_stages, net.frozen_bn            # `Network.freeze`: the first nf of FREEZE_STAGES / the trainable trunk's BatchNorms
        if nf and self.fuse_bn_bwd:
            raise L.SdError("fuse_bn_bwd does not combine with Network.freeze: its data-gradient epilogues reduce for BatchNorms that a "
                            "freeze takes out of the backward; switch one of them off")
        if amp:
            self.refresh_bf16_weights()
        x, B, H, W = self._input(x)
        rec = tape is not None
        # synchronized BatchNorm (TrainStep(sync_bn=True)): every batch-statistics finish goes through the exchange on the tape
        sx = tape.get("bn_sync") if rec else None
        if sx is not None:
            sx.begin("fwd")
        how = (self._w16, lib.sd_conv2d_fwd_bf16, None, 16, False, True) if amp \
            else (self._w32, lib.sd_conv2d_fwd, lib.sd_conv2d_fwd_workspace_bytes, 0, False, True)

        if nf:
            # frozen stages make the launches of the eval schedule (BatchNorm folded, running statistics read and not written, bf16 form
            # under mixed precision) and leave nothing on the tape
            frozen_how = self._eval_how(amp)
            p1, Hp, Wp = self._eval_stem(x, B, H, W, amp)
            if rec:
                tape["x"], tape["stem"], tape["amp"] = None, None, bool(amp)
        else:
            p1, Hp, Wp = self._train_stem(x, B, H, W, amp, sx, tape)

        # trunk (network.py:47-50)
        feats, cur, Hc, Wc = [], p1, Hp, Wp
        blocks_tape = []
        for li, layer in enumerate((net.down1, net.down2, net.down3, net.down4), start=1):
            T.push(f"fwd:down{li}")
            for blk in layer:
                if li < nf:
                    cur, Hc, Wc = self._eval_block(frozen_how, blk, cur, B, Hc, Wc)[:3]
                    continue
                if fbn:
                    # frozen BatchNorm in a trainable block: the same three launches through the training `how` (this step's weights)
                    out, Ho, Wo, a1, d1, d2, idt, dd, scales = self._eval_block(how, blk, cur, B, Hc, Wc)
                    if rec:
                        blocks_tape.append(FrozenBnRec(blk, cur, (Hc, Wc), d1, a1, d2, out, dd, idt if dd is not None else None, scales))
                    cur, Hc, Wc = out, Ho, Wo
                    continue
                c1, d1, st1 = self.conv_stats(cur, blk.conv1, B, Hc, Wc, blk.bn1, amp=amp, sync=sx)
                a1, m1, i1 = self.bn_train(c1, blk.bn1, stats=st1)
                c2, d2, st2 = self.conv_stats(a1, blk.conv2, B, d1.Ho, d1.Wo, blk.bn2, amp=amp, sync=sx)
                if blk.downsample is not None:
                    cd, dd, std_ = self.conv_stats(cur, blk.downsample[0], B, Hc, Wc, blk.downsample[1], amp=amp, sync=sx)
                    idt, md, idd = self.bn_train(cd, blk.downsample[1], relu=False, stats=std_)
                else:
                    cd = dd = md = idd = None
                    idt = cur
                out, m2, i2, msk = self.bn_train(c2, blk.bn2, res=idt, relu=True, stats=st2, want_mask=True)
                if rec:
                    blocks_tape.append(BlockRec(blk, cur, (Hc, Wc), d1, c1, a1, m1, i1, d2, c2, m2, i2, out, dd, cd, md, idd, msk))
                cur, Hc, Wc = out, d1.Ho, d1.Wo
            feats.append((cur, Hc, Wc))
            T.pop()
        (p2, H2, W2), (p3, H3, W3), (p4, H4, W4), (p5, H5, W5) = feats

        # FPN (network.py:52-55,6-19): lateral 1x1 (+bias) with the x2-upsampled coarser map added in the epilogue
        T.push("fwd:fpn")
        f, _ = self.conv(how, p5, net.up1, B, H5, W5, shift=net.up1.bias)
        fpn_tape = []
        for fpn, (sc_t, Hs, Ws) in ((net.up2, (p4, H4, W4)), (net.up3, (p3, H3, W3)), (net.up4, (p2, H2, W2))):
            t, dl = self.conv(how, sc_t, fpn.lateral, B, Hs, Ws, shift=fpn.lateral.bias, res=f, res_up2=True)
            c, dc, stf = self.conv_stats(t, fpn.conv[0], B, Hs, Ws, fpn.conv[1], amp=amp, sync=sx)
            f, mf, if_ = self.bn_train(c, fpn.conv[1], stats=stf)
            if rec:
                fpn_tape.append(FpnRec(fpn, sc_t, (Hs, Ws), dl, t, dc, c, mf, if_, f))
        T.pop()

        # head (network.py:57): NHWC -> NCHW (the head's output and the loss stay fp32)
        T.push("fwd:head")
        hc = net.head.conv
        out = torch.empty((B, hc.cout, H2, W2), dtype=torch.float32, device=x.device)
        L.check(self._fn("sd_head_fwd", amp)(f.data_ptr(), hc.weight.data_ptr(), hc.bias.data_ptr(), out.data_ptr(), B, H2 * W2, hc.cin, hc.cout,
                                             L.stream()), "sd_head_fwd")
        T.pop()
        if rec:
            tape.update(blocks=blocks_tape, fpn=fpn_tape, p5=(p5, H5, W5), f1=f, B=B, hw=(H2, W2))
        if self._nbt:
            torch._foreach_add_(self._nbt, 1)
        self._nbt = []
        return out

    def _train_stem(self, x, B, H, W, amp, sx, tape):
        """Training stem: conv7x7/2 with batch statistics, then BatchNorm + ReLU + max-pool in one pass -> (pooled map, Hp, Wp)."""
        net, lib = self.net, self.lib
        rec = tape is not None
        act = torch.bfloat16 if amp else torch.float32
        # stem: conv7x7/2 + BN + ReLU + maxpool3x3/2 (network.py:43-45)
        T.push("fwd:stem")
        stem, bn0 = net.adpater[0], net.adpater[1]
        d0 = _desc(B, H, W, stem)
        # mixed precision: the stem's conv output and pooled map are bf16 too (H % 32 == 0 makes the stem map even: the quad form of the
        # tail's backward always applies); BatchNorm statistics / arithmetic stay fp32
        s0 = torch.empty((B, d0.Ho, d0.Wo, 64), dtype=act, device=x.device)
        self._ws(lib.sd_conv2d_stem_fwd_workspace_bytes(C.byref(d0)), x.device)         # the shared workspace is at least the eval stem's
        Hp, Wp = (d0.Ho + 2 - 3) // 2 + 1, (d0.Wo + 2 - 3) // 2 + 1
        p1 = torch.empty((B, Hp, Wp, 64), dtype=act, device=x.device)
        pidx = torch.empty((B, Hp, Wp, 64), dtype=torch.uint8, device=x.device)
        # BatchNorm + ReLU + max-pool in one pass over the conv output: the full-resolution activation (1 GB at bs=64,
        # 512x512) is neither written nor read back; the backward recomputes what it needs from s0 and the pool indices
        m0 = torch.empty(64, dtype=torch.float32, device=x.device)
        i0 = torch.empty_like(m0)
        ws = self._ws(lib.sd_conv2d_stem_fwd_bn_stats_workspace_bytes(C.byref(d0)), x.device)
        if sx is None:                                                            # amp: product on the bf16 MFMA
            L.check(self._fn("sd_conv2d_stem_fwd_bn_stats", amp)(
                x.data_ptr(), stem.weight.data_ptr(), s0.data_ptr(), C.byref(d0), BN_EPS, BN_MOMENTUM, *self._running(bn0, True),
                m0.data_ptr(), i0.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "sd_conv2d_stem_fwd_bn_stats")
        else:
            sums = sx.take(64)
            sx.record("sd_conv2d_stem_fwd_bn_sums")
            L.check(self._fn("sd_conv2d_stem_fwd_bn_sums", amp)(x.data_ptr(), stem.weight.data_ptr(), s0.data_ptr(), C.byref(d0), sums.data_ptr(),
                                                                ws.data_ptr(), ws.numel(), L.stream()), "sd_conv2d_stem_fwd_bn_sums")
            self._stats_from_sums(sx, sums, bn0, m0, i0)
        self._nbt.append(bn0.num_batches_tracked)
        L.check(self._fn("sd_bn_relu_maxpool_fwd", amp)(s0.data_ptr(), B, d0.Ho, d0.Wo, 64, m0.data_ptr(), i0.data_ptr(), bn0.weight.data_ptr(),
                                                        bn0.bias.data_ptr(), p1.data_ptr(), pidx.data_ptr(), L.stream()), "sd_bn_relu_maxpool_fwd")
        if rec:
            tape["x"], tape["stem"], tape["amp"] = x, StemRec(d0, s0, m0, i0, pidx), bool(amp)
        T.pop()
        return p1, Hp, Wp

    def forward_bf16(self, x):
        """Eval-mode forward with bf16 activations / weights and fp32 accumulation; BN folded into fp32 epilogues.
        The stem reads the fp32 image with fp32 weights and stores bf16; the head returns fp32 NCHW."""
        return self._eval(x, True)

    def _eval_how(self, bf16):
        """the `how` of `conv` for the eval schedule (and for the frozen stages of a training forward)"""
        lib = self.lib
        return (self._w_bf16, lib.sd_conv2d_fwd_bf16, lib.sd_conv2d_fwd_bf16_workspace_bytes, 16, True, False) if bf16 \
            else (self._w32, lib.sd_conv2d_fwd, lib.sd_conv2d_fwd_workspace_bytes, 0, True, True)

    def _eval_stem(self, x, B, H, W, bf16):
        """Stem of the eval schedule, BatchNorm folded: conv7x7/2 + BN + ReLU + maxpool3x3/2 (network.py:43-45) -> (pooled map, Hc, Wc)."""
        net, lib = self.net, self.lib
        act = torch.bfloat16 if bf16 else torch.float32
        T.push("fwd:stem")
        stem, bn0 = net.adpater[0], net.adpater[1]
        d0 = _desc(B, H, W, stem)
        Hc, Wc = (d0.Ho + 2 - 3) // 2 + 1, (d0.Wo + 2 - 3) // 2 + 1
        cur = torch.empty((B, Hc, Wc, 64), dtype=act, device=x.device)
        one_launch = bf16 and stem.k == 7 and stem.stride == 2 and stem.pad == 3 and d0.Wo <= 4096
        if not one_launch:
            a0 = torch.empty((B, d0.Ho, d0.Wo, 64), dtype=act, device=x.device)
            wss = self._ws(lib.sd_conv2d_stem_fwd_workspace_bytes(C.byref(d0)), x.device)
        sc, sh = self.bn_fold(bn0)
        if one_launch:
            # conv1 -> bn1 -> relu -> maxpool in one launch: the (B, H/2, W/2, 64) activation is never written
            L.check(lib.sd_stem_bn_relu_maxpool_fwd_bf16(x.data_ptr(), stem.weight.data_ptr(), sc.data_ptr(), sh.data_ptr(), cur.data_ptr(),
                                                         C.byref(d0), L.stream()), "stem+maxpool")
        else:
            L.check(lib.sd_conv2d_stem_fwd(x.data_ptr(), stem.weight.data_ptr(), a0.data_ptr(), C.byref(d0), sc.data_ptr(), sh.data_ptr(), 1, int(bf16),
                                           wss.data_ptr(), wss.numel(), L.stream()), "stem")
            if bf16:
                L.check(lib.sd_maxpool3x3s2_fwd_bf16(a0.data_ptr(), cur.data_ptr(), B, d0.Ho, d0.Wo, 64, L.stream()), "maxpool")
            else:
                pidx = torch.empty((B, Hc, Wc, 64), dtype=torch.uint8, device=x.device)
                L.check(lib.sd_maxpool3x3s2_fwd(a0.data_ptr(), cur.data_ptr(), pidx.data_ptr(), B, d0.Ho, d0.Wo, 64, L.stream()), "maxpool")
        T.pop()
        return cur, Hc, Wc

    def _eval_block(self, how, blk, cur, B, Hc, Wc):
        """A BasicBlock with its BatchNorms folded into the conv epilogues: three `conv` launches (two without a downsample) ->
        (out, Ho, Wo, a1, d1, d2, idt, dd, (scale1, scale2, downsample scale or None)); the eval schedule keeps the first three."""
        s1, h1 = self.bn_fold(blk.bn1)
        a1, d1 = self.conv(how, cur, blk.conv1, B, Hc, Wc, scale=s1, shift=h1, relu=True)
        if blk.downsample is not None:
            sd_, hd = self.bn_fold(blk.downsample[1])
            idt, dd = self.conv(how, cur, blk.downsample[0], B, Hc, Wc, scale=sd_, shift=hd)
        else:
            idt, dd, sd_ = cur, None, None
        s2, h2 = self.bn_fold(blk.bn2)
        out, d2 = self.conv(how, a1, blk.conv2, B, d1.Ho, d1.Wo, scale=s2, shift=h2, res=idt, relu=True)
        return out, d1.Ho, d1.Wo, a1, d1, d2, idt, dd, (s1, s2, sd_)

    def _eval(self, x, bf16):
        """The eval schedule, fp32 or with a bf16 backbone (BASELINE stress config: "bf16 backbone + fp32 decode"): BatchNorm folded
        into the conv epilogues.  bf16 only: stem + max-pool in one launch, the head in the epilogue of the last FPN conv."""
        net, lib = self.net, self.lib
        x, B, H, W = self._input(x)
        how = self._eval_how(bf16)

        cur, Hc, Wc = self._eval_stem(x, B, H, W, bf16)

        # trunk (network.py:47-50)
        feats = []
        for li, layer in enumerate((net.down1, net.down2, net.down3, net.down4), start=1):
            T.push(f"fwd:down{li}")
            for blk in layer:
                cur, Hc, Wc = self._eval_block(how, blk, cur, B, Hc, Wc)[:3]
            feats.append((cur, Hc, Wc))
            T.pop()
        (p2, H2, W2), (p3, H3, W3), (p4, H4, W4), (p5, H5, W5) = feats

        # FPN (network.py:52-55,6-19): lateral 1x1 (+bias) with the x2-upsampled coarser map added in the epilogue
        T.push("fwd:fpn")
        f, _ = self.conv(how, p5, net.up1, B, H5, W5, shift=net.up1.bias)
        hc = net.head.conv
        out = torch.empty((B, hc.cout, H2, W2), dtype=torch.float32, device=x.device)
        for fpn, (sc_t, Hs, Ws) in ((net.up2, (p4, H4, W4)), (net.up3, (p3, H3, W3)), (net.up4, (p2, H2, W2))):
            t, _ = self.conv(how, sc_t, fpn.lateral, B, Hs, Ws, shift=fpn.lateral.bias, res=f, res_up2=True)
            sf, hf = self.bn_fold(fpn.conv[1])
            if bf16 and fpn is net.up4 and self.fuse_head and self._head_fusable(B, Hs, Ws, fpn.conv[0], hc):
                # network.py:17-18 + 22-29 in one launch where the conv takes the two-group kernel: the FPN output is never stored
                dl = _desc(B, Hs, Ws, fpn.conv[0])
                rc = lib.sd_conv2d_fwd_bf16_head(t.data_ptr(), self._w_bf16(fpn.conv[0]).data_ptr(), C.byref(dl), sf.data_ptr(), hf.data_ptr(), 1,
                                                 self._head_prepared(hc).data_ptr(), hc.cout, out.data_ptr(), L.stream())
                if rc == 0:
                    T.pop()
                    return out
                if rc > 0:
                    L.check(rc, "sd_conv2d_fwd_bf16_head")
                # rc < 0 = "geometry not served" BEFORE any launch: the remembered answer was taken under other thread-local dispatch
                # options (`conv_pp_min_tiles`, `conv_pp_strips`, `conv_fwd_split_k` change what the two-group kernel takes).  Forget
                # it and run conv + head as two launches.
                self._head_ok.pop((B, Hs, Ws, hc.cout), None)
            f, _ = self.conv(how, t, fpn.conv[0], B, Hs, Ws, scale=sf, shift=hf, relu=True)
        T.pop()

        # head (network.py:57): NHWC -> NCHW, fp32
        T.push("fwd:head")
        L.check(self._fn("sd_head_fwd", bf16)(f.data_ptr(), hc.weight.data_ptr(), hc.bias.data_ptr(), out.data_ptr(), B, H2 * W2, hc.cin, hc.cout,
                                              L.stream()), "sd_head_fwd")
        T.pop()
        return out

    # ---- bf16 backbone, inference only (BASELINE stress config: "bf16 backbone + fp32 decode") -------------
    def _w_bf16(self, conv):
        """bf16 copy of a conv weight in its physical [Cout][R][S][Cin] order (cached with the folded BN affines)."""
        key = ("w", id(conv))
        w = self.net._folded.get(key)
        if w is None:
            n = conv.weight.numel()
            w = torch.empty(n, dtype=torch.bfloat16, device=conv.weight.device)
            L.check(self.lib.sd_cast_f32_to_bf16(conv.weight.data_ptr(), w.data_ptr(), n, L.stream()), "sd_cast_f32_to_bf16")
            self.net._folded[key] = w
        return w

    def _head_fusable(self, B, Hs, Ws, conv, hc):
        """sd_conv2d_fwd_bf16_head_supported, remembered per shape (a batch-1 forward is host-bound: no descriptor + ctypes call per forward)."""
        key = (B, Hs, Ws, hc.cout)
        ok = self._head_ok.get(key)
        if ok is None:
            ok = hc.cin == 128 and bool(self.lib.sd_conv2d_fwd_bf16_head_supported(C.byref(_desc(B, Hs, Ws, conv)), hc.cout))
            self._head_ok[key] = ok
        return ok

    def _head_prepared(self, hc):
        """hi / lo bf16 halves of the fp32 head weights + the padded bias for sd_conv2d_fwd_bf16_head (cached with the folded BN affines)."""
        key = ("head", id(hc))
        buf = self.net._folded.get(key)
        if buf is None:
            buf = torch.empty(self.lib.sd_head_split_bf16_bytes(), dtype=torch.uint8, device=hc.weight.device)
            L.check(self.lib.sd_head_split_bf16(hc.weight.data_ptr(), hc.bias.data_ptr(), hc.cout, buf.data_ptr(), L.stream()), "sd_head_split_bf16")
            self.net._folded[key] = buf
        return buf

    # ---- backward ------------------------------------------------------------------------
    def _transpose_all(self, amp):
        """Every data-gradient conv's weights [Cout][taps][Cin] -> [Cin][taps][Cout] in ONE launch at the start of a backward pass
        (42 launches of ~5 us each were launch-bound: 0.24 ms per step); _wt() then hands out views until the pass ends."""
        net = self.net
        if self._wt_plan is None:
            convs = [m for m in net.modules() if isinstance(m, ConvParams) and m.cin % 64 == 0 and m.cout % 64 == 0]
            rows, views, dst, blk = [], {}, 0, 0
            for m in convs:
                taps, n = m.k * m.k, m.weight.numel()
                nbx, nby = (m.cin + 31) // 32, (m.cout + 31) // 32
                rows.append([net._flat_off[id(m.weight)][0], dst, m.cout, taps, m.cin, blk, nbx, nby])
                views[id(m)] = (dst, n)
                dst += n; blk += nbx * nby * taps
            table = torch.tensor(rows, dtype=torch.int32, device=net.flat_params.device).contiguous()
            self._wt_plan = (table, len(convs), blk, views, dst)
        table, nconv, blocks, _, total = self._wt_plan
        key = "bf16" if amp else "f32"
        if key not in self._wt_flat:
            self._wt_flat[key] = torch.empty(total, dtype=torch.bfloat16 if amp else torch.float32, device=net.flat_params.device)
        L.check(self.lib.sd_conv2d_transpose_weights_batched(net.flat_params.data_ptr(), self._wt_flat[key].data_ptr(), table.data_ptr(), nconv, blocks,
                                                             int(amp), L.stream()), "sd_conv2d_transpose_weights_batched")
        self._wt_valid = key

    def _wt(self, conv, amp=False):
        """[Cout][taps][Cin] -> [Cin][taps][Cout] for the data-gradient (amp: written as bf16 by the same pass)."""
        if self._wt_valid == ("bf16" if amp else "f32") and id(conv) in self._wt_plan[3]:
            off, n = self._wt_plan[3][id(conv)]
            return self._wt_flat[self._wt_valid][off:off + n]
        wt = torch.empty(conv.cin * conv.k * conv.k * conv.cout, dtype=torch.bfloat16 if amp else torch.float32, device=conv.weight.device)
        L.check(self._fn("sd_conv2d_transpose_weights", amp)(conv.weight.data_ptr(), wt.data_ptr(), conv.cout, conv.k * conv.k, conv.cin, L.stream()),
                "transpose_weights")
        return wt

    def _dgrad(self, dy, conv, d, res=None, bn_next=None, res_half=False, sync=None):
        """dx = dgrad(dy) [+ res] -> (dx, None).  bn_next = (x, y, relu, bn, mean, invstd) of the BatchNorm whose output gradient dx is:
        the launch then also does that BatchNorm's backward reduction (sd_conv2d_dgrad_bn_reduce) and returns (dx, the per-channel
        means) for _bn_bwd(..., means=...), which only has the apply pass left."""
        lib, amp = self.lib, dy.dtype == torch.bfloat16
        dx = torch.empty((d.B, d.Hi, d.Wi, conv.cin), dtype=dy.dtype, device=dy.device)
        wt = self._wt(conv, amp)
        head = (dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), C.byref(d))
        if bn_next is None:
            t = self._tic(d, 17 if amp else 1, amp)
            if amp:
                L.check(lib.sd_conv2d_dgrad_bf16(*head, _ptr(res), 2 if res_half else (1 if res is not None else 0), L.stream()), "sd_conv2d_dgrad_bf16")
            elif res_half:
                L.check(lib.sd_conv2d_dgrad_half_res(*head, res.data_ptr(), L.stream()), "sd_conv2d_dgrad_half_res")
            else:
                L.check(lib.sd_conv2d_dgrad(*head, _ptr(res), L.stream()), "sd_conv2d_dgrad")
            self._toc(t, d, "dgrad")
            return dx, None
        assert not amp and not res_half, "fuse_bn_bwd is an fp32-path experiment"
        x, y, relu, bn, mean, invstd = bn_next
        ws = self._ws(lib.sd_conv2d_dgrad_bn_reduce_workspace_bytes(C.byref(d)), dy.device)
        if sync is not None:            # synchronized BatchNorm: the epilogue's sums are exchanged before the means are formed
            out = sync.take(conv.cin)
            sync.record("sd_conv2d_dgrad_bn_reduce_sums")
            reduce = lib.sd_conv2d_dgrad_bn_reduce_sums
        else:
            out = torch.empty(2 * conv.cin, dtype=torch.float32, device=dy.device)
            reduce = lib.sd_conv2d_dgrad_bn_reduce
        t = self._tic(d, 1)
        L.check(reduce(*head, _ptr(res), x.data_ptr(), _mask_ptr(y, relu), relu, mean.data_ptr(), invstd.data_ptr(), bn.weight.data_ptr(),
                       bn.bias.data_ptr(), self.net.grad_of(bn.weight).data_ptr(), self.net.grad_of(bn.bias).data_ptr(), 0, out.data_ptr(),
                       ws.data_ptr(), ws.numel(), L.stream()), "sd_conv2d_dgrad_bn_reduce")
        self._toc(t, d, "dgrad")
        return dx, (out if sync is None else self._means_from_sums(sync, out, conv.cin, dy.device))

    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream()
        return self._side

    def _wgrad(self, dy, x, conv, d):
        if not self.overlap_wgrad:
            return self._wgrad_now(dy, x, conv, d)
        main, side = torch.cuda.current_stream(), self._side_stream()
        ready = torch.cuda.Event()
        ready.record(main)                       # dy (and x) are complete at this point of the main stream
        with torch.cuda.stream(side):
            side.wait_event(ready)
            self._wgrad_now(dy, x, conv, d)      # L.stream() now hands the side stream to the C ABI
        dy.record_stream(side); x.record_stream(side)

    def _join_side(self):
        if self.overlap_wgrad and self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)

    def _wgrad_now(self, dy, x, conv, d):
        g = self.net.grad_of(conv.weight)
        # mixed precision: bf16 operands, fp32 accumulation, fp32 gradient (3x3 / stride 1 layers on the bf16 MFMA through
        # transposed LDS reads; the strided and 1x1 convs widen their operands in the workspace and take the fp32 kernels)
        bf16 = dy.dtype == torch.bfloat16
        ws_bytes = self.lib.sd_conv2d_wgrad_bf16_workspace_bytes if bf16 else self.lib.sd_conv2d_wgrad_workspace_bytes
        ws = self._ws(ws_bytes(C.byref(d)), dy.device)
        t = self._tic(d, 2, bf16)
        L.check(self._fn("sd_conv2d_wgrad", bf16)(dy.data_ptr(), x.data_ptr(), g.data_ptr(), C.byref(d), 0, ws.data_ptr(), ws.numel(), L.stream()),
                "sd_conv2d_wgrad")
        self._toc(t, d, "wgrad")

    def _bias_grad(self, dy, conv):
        Mrows, Cc = dy.numel() // dy.shape[-1], dy.shape[-1]
        ws = self._ws(self.lib.sd_col_reduce_workspace_bytes(Mrows, Cc), dy.device)
        L.check(self._fn("sd_col_sum", dy.dtype == torch.bfloat16)(dy.data_ptr(), Mrows, Cc, self.net.grad_of(conv.bias).data_ptr(), 0,
                                                                   ws.data_ptr(), ws.numel(), L.stream()), "sd_col_sum")

    def _bn_bwd(self, dy, x, y, relu, bn, mean, invstd, want_g=False, means=None, sync=None):
        """BatchNorm backward: dx (and the ReLU-masked dy as `g` on request); dgamma / dbeta into the flat gradients.  means: the reduction
        was done by the data-gradient launch that produced dy, only the apply half is left.  sync: reduce half, exchange, apply half."""
        lib, bf16 = self.lib, x.dtype == torch.bfloat16
        Mrows, Cc = x.numel() // x.shape[-1], x.shape[-1]
        dx = torch.empty_like(x)
        g = torch.empty_like(x) if want_g else None
        head = (dy.data_ptr(), x.data_ptr(), _mask_ptr(y, relu), relu, Mrows, Cc, mean.data_ptr(), invstd.data_ptr(), bn.weight.data_ptr(),
                bn.bias.data_ptr())
        if means is None:
            grads = (self.net.grad_of(bn.weight).data_ptr(), self.net.grad_of(bn.bias).data_ptr(), 0)
            ws = self._ws(lib.sd_col_reduce_workspace_bytes(Mrows, Cc), x.device)
            if sync is None:
                L.check(self._fn("sd_bn_bwd", bf16)(*head, dx.data_ptr(), _ptr(g), *grads, ws.data_ptr(), ws.numel(), L.stream()), "sd_bn_bwd")
                return dx, g
            sums = sync.take(Cc)
            sync.record("sd_bn_bwd_reduce_bf16" if bf16 else "sd_bn_bwd_reduce")
            L.check(self._fn("sd_bn_bwd_reduce", bf16)(*head, *grads, sums.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "sd_bn_bwd_reduce")
            means = self._means_from_sums(sync, sums, Cc, x.device)
        L.check(self._fn("sd_bn_bwd_apply", bf16)(*head, means.data_ptr(), dx.data_ptr(), _ptr(g), L.stream()), "sd_bn_bwd_apply")
        return dx, g

    def _frozen_bwd(self, dy, y, scale, want_g=False):
        """Backward of a frozen BatchNorm (+ ReLU where `y`, its output, is given): dx = g * scale with g = dy * [y > 0]; (dx, g on request)."""
        Mrows, Cc = dy.numel() // dy.shape[-1], dy.shape[-1]
        dx = torch.empty_like(dy)
        g = torch.empty_like(dy) if want_g else None
        L.check(self._fn("sd_frozen_bn_bwd", dy.dtype == torch.bfloat16)(dy.data_ptr(), _ptr(y), scale.data_ptr(), Mrows, Cc, dx.data_ptr(), _ptr(g),
                                                                         L.stream()), "sd_frozen_bn_bwd")
        return dx, g

    def backward(self, tape, dhead, on_stage=None):
        """Writes every parameter gradient into `net.flat_grads` (overwriting, not accumulating).
        on_stage(name) is called after the gradients of a parameter group are complete, in the order
        'fpn_head', 'down4', 'down3', 'down2', 'down1_stem' (bucketed all-reduce hook).
        With `Network.freeze(stages=N)` the tape holds the trainable blocks only: the block loop ends at the first of them, which launches
        its weight-gradients but no data-gradient (its input is frozen output); lateral data-gradients into frozen output are dropped, the
        stem tail and the stem weight-gradient are not launched, and with N = 5 neither is up1's data-gradient.  Frozen slots of
        `flat_grads` are never written (`freeze` zeroed them); on_stage is still called for all five names in the same order, the frozen
        ones directly after the last trainable one."""
        net, lib = self.net, self.lib
        nf = net.frozen_stages
        if nf and self.fuse_bn_bwd:
            raise L.SdError("fuse_bn_bwd does not combine with Network.freeze; switch one of them off")
        B = tape["B"]
        H2, W2 = tape["hw"]
        dhead = dhead.contiguous().float()
        hc = net.head.conv
        amp = bool(tape.get("amp"))
        if amp and self.fuse_bn_bwd:
            raise L.SdError("fuse_bn_bwd is an fp32-path experiment; switch it off for mixed-precision training")
        sx = tape.get("bn_sync")             # synchronized BatchNorm (see forward)
        if sx is not None:
            sx.begin("bwd")
        T.push("bwd:fpn_head")
        self._transpose_all(amp)
        ws = self._ws(lib.sd_head_bwd_workspace_bytes(B, H2 * W2, hc.cin, hc.cout), dhead.device)
        # amp, narrow heads: bf16 FPN output in, bf16 gradient out (fp32 arithmetic, fp32 weight / bias gradients): no fp32 copies of the two
        # maps.  amp, wide heads: the fp32 kernels on widened copies
        widen = amp and not (hc.cin in (64, 128) and hc.cout <= 8)
        f1 = self._to_f32(tape["f1"]) if widen else tape["f1"]
        df = torch.empty_like(f1)
        L.check(self._fn("sd_head_bwd", amp and not widen)(
            dhead.data_ptr(), f1.data_ptr(), hc.weight.data_ptr(), df.data_ptr(), net.grad_of(hc.weight).data_ptr(),
            net.grad_of(hc.bias).data_ptr(), B, H2 * W2, hc.cin, hc.cout, 0, ws.data_ptr(), ws.numel(), L.stream()), "sd_head_bwd")
        if widen:
            df = self._to_bf16(df)

        # FPN, finest level first.  The lateral 1x1 data-gradients are deferred until the trunk's own
        # gradient for that tensor exists, so the sum of the two is the dgrad kernel's residual epilogue.
        lateral_grad = {}
        for r in reversed(tape["fpn"]):
            fpn, (Hs, Ws) = r.fpn, r.hw
            dcv, _ = self._bn_bwd(df, r.c, r.out, RELU_FROM_X, fpn.conv[1], r.mean, r.invstd, sync=sx)
            dt, _ = self._dgrad(dcv, fpn.conv[0], r.dc)
            self._wgrad(dcv, r.t, fpn.conv[0], r.dc)
            self._wgrad(dt, r.shortcut, fpn.lateral, r.dl)
            self._bias_grad(dt, fpn.lateral)
            lateral_grad[r.shortcut.data_ptr()] = LateralGrad(dt, fpn.lateral, r.dl)
            df = torch.empty((B, Hs // 2, Ws // 2, fpn.lateral.cout), dtype=dt.dtype, device=dt.device)
            L.check(self._fn("sd_upsample2x_bwd", amp)(dt.data_ptr(), 0, df.data_ptr(), B, Hs // 2, Ws // 2, fpn.lateral.cout, L.stream()), "up2_bwd")
        p5, H5, W5 = tape["p5"]
        d5 = _desc(B, H5, W5, net.up1)
        self._wgrad(df, p5, net.up1, d5)
        self._bias_grad(df, net.up1)
        # With `fuse_bn_bwd` every data-gradient launch that completes the gradient of a BatchNorm output also runs that
        # BatchNorm's backward reduction in its epilogue (bn_next); `mcur` / `ma1` carry the per-channel means to the apply pass.
        blocks = tape["blocks"]

        def bn2_of(i):          # bn_next tuple of block i's second BatchNorm (mask from the saved mask bytes: residual layer)
            if i < 0 or not self.fuse_bn_bwd:
                return None
            b = blocks[i]
            return (b.c2, b.mask, RELU_MASK_BYTES, b.blk.bn2, b.m2, b.i2)

        last = len(blocks) - 1
        dcur = mcur = None
        if blocks:                                              # (all five stages frozen: p5 is frozen output, nothing takes its gradient)
            has_lateral = blocks[last].out.data_ptr() in lateral_grad
            dcur, mcur = self._dgrad(df, net.up1, d5, bn_next=None if has_lateral else bn2_of(last), sync=sx)
        T.pop()
        if on_stage:
            self._join_side()
            on_stage("fpn_head")

        # trunk, last block first
        first_of = {id(net.down4[0]): "down4", id(net.down3[0]): "down3", id(net.down2[0]): "down2"}
        stage = "down4"                                         # the parameter group whose range is open
        T.push("bwd:down4")
        for bi in range(last, -1, -1):
            b = blocks[bi]
            blk, xin, (Hc, Wc) = b.blk, b.xin, b.hw
            frozen_bn = isinstance(b, FrozenBnRec)
            inner = not (nf and bi == 0)                        # False: the first trainable block behind frozen stages -- d(xin) has no taker
            extra = lateral_grad.pop(b.out.data_ptr(), None)
            if extra is not None:                       # `out` also feeds an FPN lateral conv: this launch completes d(out)
                dcur, mcur = self._dgrad(extra.dy, extra.conv, extra.d, res=dcur, bn_next=bn2_of(bi), sync=sx)
            if frozen_bn:
                s1, s2, sd_ = b.scales
                dc2, g = self._frozen_bwd(dcur, b.out, s2, want_g=True)
                da1, _ = self._dgrad(dc2, blk.conv2, b.d2)
                self._wgrad(dc2, b.a1, blk.conv2, b.d2)
                dc1, _ = self._frozen_bwd(da1, b.a1, s1)
            else:
                dc2, g = self._bn_bwd(dcur, b.c2, b.mask, RELU_MASK_BYTES, blk.bn2, b.m2, b.i2, want_g=True, means=mcur, sync=sx)
                nxt = (b.c1, None, RELU_FROM_X, blk.bn1, b.m1, b.i1) if self.fuse_bn_bwd else None
                da1, ma1 = self._dgrad(dc2, blk.conv2, b.d2, bn_next=nxt, sync=sx)
                self._wgrad(dc2, b.a1, blk.conv2, b.d2)
                dc1, _ = self._bn_bwd(da1, b.c1, b.a1, RELU_FROM_X, blk.bn1, b.m1, b.i1, means=ma1, sync=sx)
            half = False
            if blk.downsample is not None:
                if frozen_bn:
                    dcd, _ = self._frozen_bwd(g, None, sd_)
                else:
                    dcd, _ = self._bn_bwd(g, b.cd, None, RELU_NONE, blk.downsample[1], b.md, b.idd, sync=sx)
                ds, dd = blk.downsample[0], b.dd
                half = ds.k == 1 and ds.stride == 2 and ds.pad == 0 and Hc % 2 == 0 and Wc % 2 == 0 and not self.fuse_bn_bwd
                if not inner:
                    skip = None
                elif half:
                    # 1x1 / stride 2: the gradient lives on the even pixels only -> stride-1 data-gradient on the small map,
                    # joined by conv1's data-gradient epilogue (no zero-filled full-size tensor)
                    dsm = L.ConvDesc()
                    dsm.B, dsm.Hi, dsm.Wi, dsm.Cin, dsm.Cout, dsm.R, dsm.S, dsm.stride, dsm.pad = B, dd.Ho, dd.Wo, ds.cin, ds.cout, 1, 1, 1, 0
                    dsm.Ho, dsm.Wo = dd.Ho, dd.Wo
                    skip, _ = self._dgrad(dcd, ds, dsm)
                else:
                    skip, _ = self._dgrad(dcd, ds, dd)
                self._wgrad(dcd, xin, ds, dd)
            else:
                skip = g
            if inner:
                # d(xin) = d(out of the previous block), complete unless that tensor also feeds an FPN lateral (handled above)
                prev_lateral = bi > 0 and blocks[bi - 1].out.data_ptr() in lateral_grad
                nxt = None if (bi == 0 or prev_lateral) else bn2_of(bi - 1)
                dcur, mcur = self._dgrad(dc1, blk.conv1, b.d1, res=skip, bn_next=nxt, res_half=half, sync=sx)
            self._wgrad(dc1, xin, blk.conv1, b.d1)
            if id(blk) in first_of:                                         # the first block of a layer closes that layer's range
                T.pop()
                if on_stage:
                    self._join_side()
                    on_stage(first_of[id(blk)])
                stage = {"down4": "down3", "down3": "down2", "down2": "down1_stem"}[first_of[id(blk)]]
                T.push("bwd:" + stage)

        lateral_grad.clear()                                    # what is left points into frozen output: dropped on purpose
        if nf:
            # frozen stages: no stem tail, no stem weight-gradient; the open range closes and the remaining (frozen, all-zero) parameter
            # groups are reported in today's order, so that the bucket plans of the exchange stay as they are
            self._join_side()
            self._wt_valid = None
            T.pop()
            if on_stage:
                names = ("down4", "down3", "down2", "down1_stem")
                for name in names[names.index(stage):]:
                    on_stage(name)
            return

        # stem (H % 32 == 0 made its map even: under mixed precision the conv output and the pooled gradient are bf16, as autocast's conv1
        # backward sees them)
        stem, bn0 = net.adpater[0], net.adpater[1]
        d0, s0, m0, i0, pidx = tape["stem"]
        ring = amp and self.stem_ring and d0.Wi % 4 == 0          # the row-ring weight gradient fetches the image in aligned groups of four columns
        # amp: the products on the bf16 MFMA (autocast: conv1 in bf16); ring: a bf16 stem gradient for the row-ring weight-gradient kernel
        pool_bwd, pool_reduce, pool_apply, stem_wgrad = {
            (False, False): (lib.sd_maxpool_bn_relu_bwd, lib.sd_maxpool_bn_relu_bwd_reduce, lib.sd_maxpool_bn_relu_bwd_apply, lib.sd_conv2d_stem_wgrad),
            (True, False): (lib.sd_maxpool_bn_relu_bwd_bf16, lib.sd_maxpool_bn_relu_bwd_reduce_bf16, lib.sd_maxpool_bn_relu_bwd_apply_bf16,
                            lib.sd_conv2d_stem_wgrad_bf16mm),
            (True, True): (lib.sd_maxpool_bn_relu_bwd_bf16_dx16, lib.sd_maxpool_bn_relu_bwd_reduce_bf16, lib.sd_maxpool_bn_relu_bwd_apply_bf16_dx16,
                           lib.sd_conv2d_stem_wgrad_bf16)}[amp, ring]
        ds0 = torch.empty(s0.shape, dtype=torch.bfloat16 if ring else torch.float32, device=s0.device)
        ws = self._ws(lib.sd_col_reduce_workspace_bytes(B * d0.Ho * d0.Wo, 64), s0.device)
        head = (dcur.data_ptr(), pidx.data_ptr(), s0.data_ptr(), B, d0.Ho, d0.Wo, 64, m0.data_ptr(), i0.data_ptr(), bn0.weight.data_ptr(),
                bn0.bias.data_ptr())
        grads = (net.grad_of(bn0.weight).data_ptr(), net.grad_of(bn0.bias).data_ptr(), 0)
        if sx is None:
            L.check(pool_bwd(*head, ds0.data_ptr(), *grads, ws.data_ptr(), ws.numel(), L.stream()), "sd_maxpool_bn_relu_bwd")
        else:                                         # synchronized BatchNorm: reduce half, exchange, means, apply half
            sums = sx.take(64)
            sx.record("sd_maxpool_bn_relu_bwd_reduce")
            L.check(pool_reduce(*head, *grads, sums.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "sd_maxpool_bn_relu_bwd_reduce")
            means = self._means_from_sums(sx, sums, 64, s0.device)
            L.check(pool_apply(*head, means.data_ptr(), ds0.data_ptr(), L.stream()), "sd_maxpool_bn_relu_bwd_apply")
        ws = self._ws(lib.sd_conv2d_stem_wgrad_workspace_bytes(C.byref(d0)), ds0.device)
        L.check(stem_wgrad(ds0.data_ptr(), tape["x"].data_ptr(), net.grad_of(stem.weight).data_ptr(), C.byref(d0), 0,
                           ws.data_ptr(), ws.numel(), L.stream()), "sd_conv2d_stem_wgrad")
        self._join_side()
        self._wt_valid = None                               # the optimizer step that follows changes the weights
        T.pop()
        if on_stage:
            on_stage("down1_stem")


class _NetFn(torch.autograd.Function):
    """One autograd node for the whole network: inputs = image + every parameter."""

    @staticmethod
    def forward(ctx, net, x, *params):
        tape = {}
        out = net._engine.forward(x, True, tape)
        ctx.net, ctx.tape = net, tape
        return out

    @staticmethod
    def backward(ctx, dhead):
        net = ctx.net
        net._engine.backward(ctx.tape, dhead)
        ctx.tape = None
        return (None, None) + tuple(None if id(p) in net._frozen_ids else net.grad_of(p) for p in net._flat_order)


class Network(nn.Module):
    def __init__(self, args, pretrained=True, raw_output: bool = False, init_weights: bool = True):
        """network.py:33.  `init_weights=False` (extension): leave the parameters uninitialised -- for callers that load a complete
        state_dict right away (`evaluate`, `detect`, `Predictor`: the seeded random init of 21.8 M values is 0.1-0.6 s of their start-up)."""
        super().__init__()
        self.raw_output = raw_output
        # bf16 backbone for the eval-mode forward (BASELINE stress config: "bf16 backbone + fp32 decode"): `--bf16_inference`, or
        # `--amp` -- the reference autocasts its validation forward under that flag too (trainer.py:141-155).  What `--amp` means
        # for the TRAINING step (trainer.py:115-121) is decided by the Trainer, not here.
        self.bf16_inference = bool(getattr(args, "use_amp", False) or getattr(args, "bf16_inference", False))
        self.label_count = len(args.labels)  # M
        self.part_count = len(args.parts)  # N
        self.out_channels = self.label_count + self.part_count + 4
        self.fpn_depth = args.fpn_depth
        if self.fpn_depth % 64:
            raise L.SdError("fpn_depth must be a multiple of 64 for the MFMA tiles")
        if self.out_channels > 256:
            raise L.SdError(f"labels + parts + 4 must be <= 256 (head kernel limit SD_HEAD_MAX_CO); got {self.out_channels}")
        if self.out_channels > 32 and self.fpn_depth not in (64, 128, 256):
            raise L.SdError(f"labels + parts + 4 > 32 needs fpn_depth in (64, 128, 256) (the wide head kernels); got {self.fpn_depth}")

        self.adpater = nn.Sequential(ConvParams(3, 64, 7, 2, 3), BNParams(64), Slot(), Slot())   # sic (network.py:43)
        self.down1 = _layer(64, 64, 3, 1)
        self.down2 = _layer(64, 128, 4, 2)
        self.down3 = _layer(128, 256, 6, 2)
        self.down4 = _layer(256, 512, 3, 2)
        self.up1 = ConvParams(512, self.fpn_depth, 1, bias=True)
        self.up2 = Fpn(256, self.fpn_depth)
        self.up3 = Fpn(128, self.fpn_depth)
        self.up4 = Fpn(64, self.fpn_depth)
        self.head = Head(self.fpn_depth, self.out_channels)
        if init_weights:
            self.reset_parameters(seed=0)
        # network.py:41: `resnet34(weights=ResNet34_Weights.DEFAULT if pretrained else None)` -- the ImageNet trunk.  torchvision would
        # download `resnet34-b627a593.pth` into the hub cache; here the file is looked up locally (no download): `--backbone_weights`,
        # $SDNET_BACKBONE_WEIGHTS, then torchvision's own cache locations.  Not finding it is announced loudly: the run then starts
        # from a different model than the reference's.
        self.backbone_weights = None
        if pretrained:
            path = find_backbone_weights(args)
            if path is None:
                warnings.warn(
                    "Network(pretrained=True): no ImageNet ResNet-34 checkpoint found -- the trunk starts from RANDOM weights, unlike "
                    "the reference (network.py:41).  Pass --backbone_weights /path/to/resnet34-b627a593.pth (torchvision's "
                    "ResNet34_Weights.DEFAULT state_dict), set SDNET_BACKBONE_WEIGHTS, or place the file in "
                    "$TORCH_HOME/hub/checkpoints/.", RuntimeWarning, stacklevel=2)
            else:
                self.load_backbone_state_dict(torch.load(path, map_location="cpu", weights_only=True))
                self.backbone_weights = str(path)
        self.flat_params = self.flat_grads = self.flat_params_bf16 = None
        self._flat_order, self._flat_off = [], {}
        self._folded = {}        # eval-mode (scale, shift) per BN, valid until the parameters can have changed
        self._engine = None
        self.frozen_stages, self.frozen_bn, self._frozen_ids = 0, False, frozenset()      # fine-tuning: `freeze`

    # ---- init / flat storage -------------------------------------------------------------
    def reset_parameters(self, seed=0):
        """torchvision's scheme: kaiming_normal_(fan_out, relu) for convs, BN weight 1 / bias 0;
        torch default (kaiming_uniform a=sqrt(5)) for the biased FPN / head convs."""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, ConvParams):
                    fan_out = m.cout * m.k * m.k
                    fan_in = m.cin * m.k * m.k
                    if m.bias is None:
                        m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / fan_out))
                    else:
                        bound = 1.0 / math.sqrt(fan_in)
                        m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 2 - 1) * bound)
                        m.bias.copy_((torch.rand(m.bias.shape, generator=g) * 2 - 1) * bound)

    def _apply(self, fn, *a, **kw):
        super()._apply(fn, *a, **kw)
        self._build_flat()
        return self

    def _build_flat(self):
        """Move every parameter into one flat buffer (16-byte aligned slots) and alias it."""
        params = [p for p in self.parameters()]
        if not params or not params[0].is_cuda:
            self.flat_params = self.flat_grads = None
            return
        dev = params[0].device
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 7) // 8 * 8          # 32-byte slots: the bf16 view of a conv weight (same element offset, _w16) stays 16-byte aligned
        flat = torch.zeros(total, dtype=torch.float32, device=dev)
        grads = torch.zeros(total, dtype=torch.float32, device=dev)
        self._flat_order, self._flat_off = params, {}
        with torch.no_grad():
            for p, off in zip(params, offs):
                n = p.numel()
                if p.dim() == 4:                      # physical [Cout][R][S][Cin], logical OIHW
                    co, ci, r, s = p.shape
                    view = flat[off:off + n].view(co, r, s, ci).permute(0, 3, 1, 2)
                else:
                    view = flat[off:off + n].view(p.shape)
                view.copy_(p.data)
                p.data = view
                self._flat_off[id(p)] = (off, n)
        self.flat_params, self.flat_grads, self.flat_params_bf16 = flat, grads, None
        self._folded = {}
        self._engine = _Engine(self)                         # (a freeze survives: the parameters are the same objects, the new gradients are zero)

    # ---- fine-tuning: frozen trunk stages, frozen BatchNorm ------------------------------------
    def freeze(self, stages=0, bn=False):
        """Fine-tuning (`train --freeze_stages N [--freeze_bn]`), callable before or after `.to(device)`; `freeze(0)` undoes it.
        stages = N: the first N of FREEZE_STAGES (stem, down1 .. down4), as Detectron2's FREEZE_AT -- their convolution weights and
        BatchNorm weight / bias get no gradient and never change (`requires_grad = False`), their BatchNorms normalise with the running
        statistics and write neither those nor `num_batches_tracked`; the training forward runs them on the eval schedule and the backward
        does not visit them.  bn = True (needs N >= 1): the BatchNorms of the trunk blocks that still train are FrozenBatchNorm2d --
        running statistics used and not written, weight / bias fixed, the convolutions around them train; the FPN's BatchNorms keep batch
        statistics.  Eval-mode forwards and the state_dict keys are unchanged.  The frozen slots of `flat_grads` are zeroed here and
        never written afterwards: the frozen stages are the prefix `frozen_range()` of the flat buffers."""
        if isinstance(stages, bool) or not isinstance(stages, int) or not 0 <= stages <= len(FREEZE_STAGES):
            raise ValueError(f"freeze: stages should be an integer in [0, {len(FREEZE_STAGES)}], not {stages!r}")
        if bn and stages == 0:
            raise ValueError("freeze: bn=True needs stages >= 1 (a frozen stem BatchNorm behind a trainable stem is not built)")
        self.frozen_stages, self.frozen_bn = int(stages), bool(bn)
        self._folded = {}                                    # a layer frozen now may have trained since its fold / bf16 copy was cached
        self._mark_frozen()
        return self

    def _frozen_parameters(self):
        """the parameters a freeze fixes: everything of the frozen stages, and under `frozen_bn` the BatchNorm weight / bias of the rest of the trunk"""
        out = []
        for k, name in enumerate(FREEZE_STAGES):
            stage = getattr(self, name)
            if k < self.frozen_stages:
                out += list(stage.parameters())
            elif self.frozen_bn:
                out += [p for m in stage.modules() if isinstance(m, BNParams) for p in m.parameters()]
        return out

    def _mark_frozen(self):
        frozen = self._frozen_parameters()
        self._frozen_ids = frozenset(id(p) for p in frozen)
        for p in self.parameters():
            p.requires_grad_(id(p) not in self._frozen_ids)
        if self.flat_grads is not None:
            for p in frozen:
                off, n = self._flat_off[id(p)]
                self.flat_grads[off:off + n].zero_()

    def frozen_range(self):
        """(0, off): the flat-buffer element range of the frozen stages -- a prefix, because FREEZE_STAGES is the order of parameters();
        off is the start of the first trainable stage's first slot (slots as `_build_flat` lays them out: 8 floats each)."""
        return 0, sum((p.numel() + 7) // 8 * 8 for name in FREEZE_STAGES[:self.frozen_stages] for p in getattr(self, name).parameters())

    def optim_groups(self):
        """Parameter groups of the optimizer for per-stage learning rates (`TrainStep(lr_mults=...)`, sd_optim_groups_step):
        (ids, groups).  `groups[k]` = (stage, decayed) for group id k: the stages of OPTIM_STAGES in flat-buffer order, each split into
        its 4-D tensors (convolution weights: decayed, what `TrainStep.build_decay_mask` flags) and the rest (biases, BatchNorm weight /
        bias) -- 14 groups, id = 2 * stage index + decayed.  `ids`: a uint8 host tensor with one byte per group of four floats of the flat
        buffer (`flat_params.numel() // 4`; the layout of `_build_flat`, so it can be asked for before `.to(device)`); the padding of a
        32-byte slot carries the id of its tensor."""
        groups = [(stage, decayed) for stage in OPTIM_STAGES for decayed in (False, True)]
        stage_of = {}
        for k, stage in enumerate(OPTIM_STAGES):
            for name in (("up1", "up2", "up3", "up4") if stage == "fpn" else (stage,)):
                for p in getattr(self, name).parameters():
                    stage_of[id(p)] = k
        params = list(self.parameters())
        ids = torch.zeros(sum((p.numel() + 7) // 8 * 8 for p in params) // 4, dtype=torch.uint8)
        off = 0
        for p in params:                                     # `_build_flat`: registration order, 8-float slots
            slot = (p.numel() + 7) // 8 * 8
            ids[off // 4:(off + slot) // 4] = 2 * stage_of[id(p)] + int(p.dim() == 4)
            off += slot
        assert self.flat_params is None or ids.numel() * 4 == self.flat_params.numel()
        return ids, groups

    def optim_slots(self):
        """The slot table of the layer-wise optimizer (`TrainStep(optimizer="lamb")`, sd_lamb_step): one (lo, hi, adapt) per parameter,
        in flat-buffer order.  [lo, hi) is the parameter's 8-float slot in floats (the layout of `_build_flat`, padding included, so it
        can be asked for before `.to(device)`); the slots tile the buffer like the ids of `optim_groups()`.  adapt: the slot's step is
        scaled by its trust ratio -- True for 4-D tensors (convolution weights, the tensors `optim_groups()` marks as decayed), False
        for biases and BatchNorm weight / bias."""
        slots, off = [], 0
        for p in self.parameters():                          # `_build_flat`: registration order, 8-float slots
            hi = off + (p.numel() + 7) // 8 * 8
            slots.append((off, hi, p.dim() == 4))
            off = hi
        assert self.flat_params is None or off == self.flat_params.numel()
        return slots

    def grad_of(self, p):
        off, n = self._flat_off[id(p)]
        g = self.flat_grads[off:off + n]
        if p.dim() == 4:
            co, ci, r, s = p.shape
            return g.view(co, r, s, ci).permute(0, 3, 1, 2)
        return g.view(p.shape)

    def invalidate_folded(self):
        """Drop the cached eval-mode BN affines (call after editing parameters in place while in eval mode)."""
        self._folded = {}

    def train(self, mode=True):
        self._folded = {}
        return super().train(mode)

    def load_state_dict(self, *a, **kw):
        self._folded = {}
        return super().load_state_dict(*a, **kw)

    def load_backbone_state_dict(self, resnet_sd):
        """Copy a torchvision ResNet-34 state_dict (keys `conv1.weight`, `bn1.*`, `layer{1..4}.{b}.*`, `fc.*`) onto the trunk, the way
        network.py:41-50 picks the sub-modules: conv1 / bn1 -> `adpater.0` / `adpater.1`, layerL -> `downL`; `fc.*` is dropped (the
        reference never registers it).  Strict on the trunk: every trunk tensor must be present with the right shape, and nothing
        but `fc.*` may be left over.  FPN and head keep their initialisation, as in the reference."""
        mapped, extra = {}, []
        for k, v in resnet_sd.items():
            if k.startswith("fc."):
                continue
            if k.startswith("conv1."):
                mapped["adpater.0." + k[len("conv1."):]] = v
            elif k.startswith("bn1."):
                mapped["adpater.1." + k[len("bn1."):]] = v
            elif k.startswith("layer") and k[5:6] in "1234" and k[6:7] == ".":
                mapped["down" + k[5:]] = v
            else:
                extra.append(k)
        own = self.state_dict()
        trunk = [k for k in own if k.split(".")[0] in ("adpater", "down1", "down2", "down3", "down4")]
        missing = [k for k in trunk if k not in mapped]
        extra += [k for k in mapped if k not in own]
        bad = [f"{k}: {tuple(mapped[k].shape)} != {tuple(own[k].shape)}" for k in trunk if k in mapped and mapped[k].shape != own[k].shape]
        if missing or extra or bad:
            raise L.SdError(f"not a torchvision ResNet-34 state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                            f"unexpected {extra[:4]}, shape mismatches {bad[:4]}")
        self._folded = {}
        with torch.no_grad():
            for k in trunk:
                own[k].copy_(mapped[k])
        return len(trunk)

    # ---- reference API -------------------------------------------------------------------
    def forward(self, x):  # (B, 3, H, W)
        if self._engine is None:
            raise L.SdError("Network must be moved to the GPU first (`net.to('cuda')`): there is no CPU path")
        if self.training and torch.is_grad_enabled():
            out = _NetFn.apply(self, x, *self._flat_order)
        elif self.bf16_inference and not self.training:
            out = self._engine.forward_bf16(x)
        else:
            out = self._engine.forward(x, self.training)
        if self.raw_output:
            return out
        M, nb = self.label_count, self.label_count + self.part_count
        return {"anchor_hm": out[:, :M], "part_hm": out[:, M:nb], "offsets": out[:, nb:nb + 2], "embeddings": out[:, nb + 2:nb + 4]}

    def save(self, path="last_model.pth"):
        torch.save({k: v.clone() for k, v in self.state_dict().items()}, path)

    # ---- hipGraph replay of the eval forward (launch-bound small batches) --------------------
    def graphed(self, example: torch.Tensor):
        """Capture the eval-mode forward for `example`'s shape into a hipGraph and return `run(x) -> head tensor`.
        Input and output buffers are static (the returned tensor is overwritten by the next call; write into `run.static_in` to skip the
        input copy).  Measured (tools/graph_vs_eager.sh, round 4): at bs=1 the eager stream is already gap-free -- the host enqueues ahead and
        the 44 kernels run back to back (sum of kernel durations = wall time) -- so a replay has no launch gaps to remove and adds its own
        fixed cost (the copy launch + ~9 us between replays): use it when the HOST is the bottleneck (a busy Python thread), not for speed."""
        if self.training:
            raise L.SdError("graphed() captures the inference forward: call net.eval() first")
        static_in = example.detach().clone().contiguous().float()
        # the forward `net(x)` would run: the bf16 backbone when `bf16_inference` is set (captured as it is NOW: capture again after a change)
        fwd = self._engine.forward_bf16 if self.bf16_inference else (lambda t: self._engine.forward(t, False))
        with torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):           # warm-up on the capture stream: allocations, one-time attributes
                for _ in range(2):
                    fwd(static_in)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                static_out = fwd(static_in)

        def run(x):
            if x.data_ptr() != static_in.data_ptr():      # a caller that fills `run.static_in` itself saves the copy launch
                static_in.copy_(x, non_blocking=True)
            graph.replay()
            return static_out

        run.graph, run.static_in, run.static_out = graph, static_in, static_out
        return run

    # ---- explicit (autograd-free) training path used by the trainer / bench ----------------
    def forward_train(self, x, amp=False, bn_sync=None):
        """Forward in training mode recording the tape; returns (head tensor, tape).  amp=True: the mixed-precision step of the
        reference's `--amp` (trainer.py:115-121) -- bf16 activations and conv weights, fp32 accumulation, statistics and master weights.
        bn_sync (a `sync_bn.BnStatsExchange`): synchronized BatchNorm -- every BatchNorm of this forward and of `backward_from(tape, ...)`
        finishes its batch statistics through the exchange (global statistics over the ranks of its process group).  None: today's launches."""
        tape = {} if bn_sync is None else {"bn_sync": bn_sync}
        return self._engine.forward(x, True, tape, amp=amp), tape

    def backward_from(self, tape, dhead, on_stage=None):
        """Backward of `forward_train`: fills `flat_grads` in place."""
        self._engine.backward(tape, dhead, on_stage)

    def stage_ranges(self):
        """Flat-buffer [lo, hi) element ranges of the gradient groups reported by `backward_from(on_stage=...)`."""
        def span(mods):
            offs = [self._flat_off[id(p)] for m in mods for p in m.parameters()]
            return (min(o for o, _ in offs), max((o + n + 7) // 8 * 8 for o, n in offs))
        return {"fpn_head": span([self.up1, self.up2, self.up3, self.up4, self.head]), "down4": span([self.down4]),
                "down3": span([self.down3]), "down2": span([self.down2]), "down1_stem": span([self.adpater, self.down1])}
