"""Training step and loop for the SDNet hot path.

`TrainStep` is the inner step of the reference's `Trainer.train_epoch`
(src/sdnet/model/trainer.py:113-124: zero_grad, forward, loss, backward, Adam.step with lr 1e-3 and
default betas/eps, :53) as an explicit kernel schedule with no host synchronisation, extended with
what the reference lacks: pure data-parallel training, one process per GPU, gradients summed with
RCCL (`torch.distributed` backend "nccl") in five buckets that follow the backward pass
(FPN+head, down4, down3, down2, down1+stem), so the 87 MB exchange hides behind the remaining
backward kernels; the mean is applied inside the fused Adam launch (grad_scale = 1/world).
BatchNorm statistics are rank-local by default; `sync_bn=True` (`train --sync_bn`) computes them over the global batch
(model/sync_bn.py) through the same process group as the gradient buckets.
`accum_steps=K` (`train --accum_steps K`) makes one optimizer step of K consecutive batches: `sd_grad_accum` folds each bucket into an
accumulator as the backward completes it, and the exchange and the optimizer run once per K calls (grad_scale = 1/(K world)).
"""
from __future__ import annotations

import os
from contextlib import contextmanager

import torch
import torch.distributed as dist

from .. import _lib as L
from ..utils import trace as T
from .loss import LossStats, loss_backward, loss_config, loss_forward


BF16_TRAINING = True       # `--amp`: bf16 activations / conv weights, fp32 accumulation + master weights (autocast semantics of trainer.py:115-121)


class RcclExchange:
    """Gradient sum straight through the C ABI (`sd_allreduce_*`, RCCL): what a host without torch.distributed would
    call.  The 128-byte RCCL id travels over the already initialised process group's store (any host channel works);
    each bucket's all-reduce runs on a side stream that first waits for the compute stream (so it is ordered after the
    weight-gradient kernels issued so far) and `wait()` joins it back before the Adam launch.  Opt-in
    (`TrainStep(..., exchange="rccl")` or SDNET_EXCHANGE=rccl); the default exchange is torch.distributed's RCCL binding."""

    def __init__(self, device, process_group=None):
        import ctypes as C
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
        ident = C.create_string_buffer(128)
        if rank == 0:
            L.check(L.lib().sd_allreduce_unique_id(ident), "sd_allreduce_unique_id")
        box = [ident.raw if rank == 0 else None]
        dist.broadcast_object_list(box, src=0, group=process_group)
        ident = C.create_string_buffer(box[0], 128)
        self._comm = C.c_void_p()
        with torch.cuda.device(device):
            L.check(L.lib().sd_allreduce_init(ident, rank, world, C.byref(self._comm)), "sd_allreduce_init")
        self.world = world
        self.side = torch.cuda.Stream(device)

    def all_reduce(self, flat, lo, hi):
        self.side.wait_stream(torch.cuda.current_stream())
        L.check(L.lib().sd_allreduce_run(self._comm, flat.data_ptr() + 4 * lo, hi - lo, self.side.cuda_stream), "sd_allreduce_run")

    def wait(self):
        torch.cuda.current_stream().wait_stream(self.side)

    def close(self):
        if self._comm:
            L.check(L.lib().sd_allreduce_destroy(self._comm), "sd_allreduce_destroy")
            self._comm = None


class SimExchange:
    """Stand-in for the gradient all-reduce on ONE GPU (`TrainStep(..., exchange="sim")`): at every bucket trigger point of the backward a
    persistent copy launch of RCCL's shape (`sd_comm_sim_copy`: `workgroups` blocks of 256 threads, 8 KB of LDS, link-bound at `gbps`) moves
    2 (N - 1) / N x the bucket (N = `ranks`) on the exchange's side stream -- same ordering as `RcclExchange` (waits for the compute stream,
    joined before Adam).  The gradients are NOT changed (the copy goes to a scratch buffer): the step computes what a single rank computes;
    only its timing carries the collective's footprint.  bench.py: `north_star.comm_sim`."""

    def __init__(self, device, largest_bucket_floats, ranks=8, workgroups=32, gbps=200.0):
        self.ranks, self.workgroups, self.gbps = int(ranks), int(workgroups), float(gbps)
        self.side = torch.cuda.Stream(device)
        self.scratch = torch.empty(largest_bucket_floats, dtype=torch.float32, device=device)
        self.moved_bytes = 0

    def all_reduce(self, flat, lo, hi):
        n = hi - lo
        if n > self.scratch.numel():
            raise L.SdError(f"SimExchange: bucket of {n} floats exceeds the scratch buffer ({self.scratch.numel()})")
        move = int(2 * (self.ranks - 1) / self.ranks * n * 4) // 16 * 16
        self.side.wait_stream(torch.cuda.current_stream())
        L.check(L.lib().sd_comm_sim_copy(flat.data_ptr() + 4 * lo, self.scratch.data_ptr(), n * 4, move, self.workgroups, self.gbps, self.side.cuda_stream),
                "sd_comm_sim_copy")
        self.moved_bytes += move

    def wait(self):
        torch.cuda.current_stream().wait_stream(self.side)


class TrainStep:
    """One optimizer step on the flat buffers.  Fine-tuning: the net's `freeze` setting is read HERE, at construction (freeze first, then
    build the step).  The optimizer then works on the suffix `flat[off:]` behind the frozen stages (`Network.frozen_range()`): parameter,
    gradient, both moments and the EMA are offset by `off`, the decay mask by off / 4 bytes, n = total - off (slots are 32-byte aligned, so
    every alignment rule holds) -- the prefix is never written by decay, update or average.  Frozen BatchNorm weight / bias INSIDE the
    suffix (`freeze(bn=True)`) stay fixed because their gradient and their moments are zero, which makes the Adam update exactly zero and
    leaves them undecayed (the mask covers convolution weights only): `Network.freeze` zeroes those slots of `flat_grads` and the backward
    never writes them; their `exp_avg` / `exp_avg_sq` slots are zeroed at construction and again after `load_state_dict`.

    Gradient accumulation (`accum_steps=K`, `train --accum_steps K`, 1 .. 64; torch's accumulation loop): a call is one MICRO-step -- a
    normal training forward (batch statistics of that batch, one momentum update of the running statistics, `sync_bn` all-reduces as
    always), that batch's loss with its own normalisation, and the plain backward into `flat_grads`.  As each of the five parameter
    groups completes, one `sd_grad_accum` launch on the step's stream folds it into `grad_acc` (micro-step 1 overwrites, 2 .. K - 1
    add); on micro-step K the launch adds `grad_acc` into `flat_grads` instead, and only then does that group's gradient exchange start.
    `flat_grads` then holds (((g1 + g2) + ...) + gK) in fp32, the gradients are exchanged once per optimizer step, and the optimizer
    runs with grad_scale = 1 / (K * world): the mean of the micro-batch gradients (not the gradient of one large batch: every
    micro-loss divides by its own batch's counts).  `updated` tells whether the call ran the optimizer; `step_count` counts optimizer
    steps.  `flush()` ends a partial group (the end of an epoch) with the mean over what it holds.  With K = 1 nothing of this exists:
    no buffer, no launch, the step as it always was.  Neither buffer is read or written below `frozen_off`.

    `optimizer` picks the update rule ("adam", the default and the step as it always was; "sgd": torch.optim.SGD with `momentum` and
    `nesterov`, dampening 0, sd_sgd_step; "lamb": LAMB with the trust ratio on convolution weights, sd_lamb_step).  The two new rules
    always run in the groups form -- `Network.optim_groups()` ids, a uniform rate table when `lr_mults` is None -- and take every
    option above unchanged.  Under sgd `weight_decay` is COUPLED L2 (it enters the gradient and the momentum), `exp_avg` is the momentum
    buffer and `exp_avg_sq` is None; lamb keeps both moments and adds the network's slot table (`Network.optim_slots()`, uploaded once)
    and a few KB of fp64 partials.  No accuracy is claimed for either: the update rules are tested, not trained models."""

    MAX_ACCUM_STEPS = 64
    OPTIMIZERS = ("adam", "sgd", "lamb")

    def __init__(self, net, args, lr=None, betas=(0.9, 0.999), eps=1e-8, process_group=None, exchange=None, sync_bn=False,
                 weight_decay=0.0, clip_grad_norm=0.0, ema_decay=0.0, lr_mults=None, accum_steps=1, optimizer="adam", momentum=0.9, nesterov=False):
        if net.flat_params is None:
            raise L.SdError("move the Network to the GPU before building TrainStep")
        if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or not 1 <= accum_steps <= self.MAX_ACCUM_STEPS:
            raise ValueError(f"accum_steps must be an integer in [1, {self.MAX_ACCUM_STEPS}], got {accum_steps!r}")
        if weight_decay < 0 or clip_grad_norm < 0 or not 0 <= ema_decay < 1:
            raise ValueError(f"weight_decay and clip_grad_norm must be >= 0 and ema_decay in [0, 1), got {weight_decay!r}, {clip_grad_norm!r}, "
                             f"{ema_decay!r}")
        if optimizer not in self.OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {', '.join(self.OPTIMIZERS)}, got {optimizer!r}")
        if not 0 <= momentum < 1:                            # (false for nan)
            raise ValueError(f"momentum must be in [0, 1), got {momentum!r}")
        if optimizer == "sgd" and nesterov and momentum == 0:
            raise ValueError("nesterov needs momentum > 0")
        self.optimizer, self.momentum, self.nesterov = optimizer, float(momentum), bool(nesterov)
        self.lr_mults = self.check_lr_mults(lr_mults)
        self.net, self.args = net, args
        self.lr = float(lr if lr is not None else getattr(args, "learning_rate", 1e-3))
        self.betas, self.eps = betas, eps
        self.exp_avg = torch.zeros_like(net.flat_params)
        self.exp_avg_sq = torch.zeros_like(net.flat_params) if optimizer != "sgd" else None      # sgd: one state buffer (the momentum)
        self.frozen = (int(getattr(net, "frozen_stages", 0)), bool(getattr(net, "frozen_bn", False)))
        self.frozen_off = net.frozen_range()[1] if self.frozen[0] else 0          # the optimizer's range starts behind the frozen stages
        self._zero_frozen_moments()
        self.step_count = 0
        # gradient accumulation: the running sum of the group's micro-batch gradients (only with K > 1), the micro-steps taken in the
        # current group, and whether the last call ran the optimizer
        self.accum_steps = accum_steps
        self.grad_acc = torch.zeros_like(net.flat_grads) if accum_steps > 1 else None
        self.micro, self.updated = 0, False
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        exchange = exchange or os.environ.get("SDNET_EXCHANGE", "torch")
        want_sim = exchange == "sim"
        if exchange not in ("torch", "rccl", "sim"):
            raise ValueError(f"exchange must be 'torch', 'rccl' or 'sim', got {exchange!r}")
        if sync_bn and exchange == "rccl":
            # the statistics would need a second communicator beside the C-ABI one: two communicators whose collectives can run in
            # different orders on different ranks can deadlock the GPUs
            raise L.SdError("sync_bn needs the torch.distributed exchange: its statistics all-reduces must share the gradient buckets' "
                            "process group (one communicator, one order on every rank); exchange='rccl' is a communicator of its own")
        self.rccl = RcclExchange(net.flat_params.device, process_group) if (exchange == "rccl" and self.world > 1) else None
        self.ranges = net.stage_ranges()
        self.sim = None                  # SimExchange: the collective's footprint on one GPU (attach_sim)
        if want_sim:
            self.attach_sim()
        self.one = torch.ones((), dtype=torch.float32, device=net.flat_params.device)
        self.stats = LossStats()
        self.amp = bool(getattr(args, "use_amp", False))      # mixed-precision step (trainer.py:115-121)
        self.exchange_enabled = True     # False: skip the all-reduce (bench.py measures the exposed communication time with it)
        # synchronized BatchNorm: per-layer fp64 statistics all-reduced over `process_group` (the gradient buckets' group); with one
        # rank the split finish runs without a collective (bit-identical to the default step)
        self.sync_bn = bool(sync_bn)
        self.bn_sync = None
        if self.sync_bn:
            from .sync_bn import BnStatsExchange
            self.bn_sync = BnStatsExchange.for_network(net, process_group, self.world)
        # large-batch options of the optimizer (sd_optim_step): all zero = the plain sd_adam_step launch.  The status block
        # ([0] float norm, [1] float clip coefficient, [2] int32 skipped steps) lives on the device and is never read by the step.
        self.weight_decay, self.clip_grad_norm, self.ema_decay = float(weight_decay), float(clip_grad_norm), float(ema_decay)
        self.decay_mask = self.ema = self._partials = self.group_ids = self._lamb = None
        self._status = torch.zeros(4, dtype=torch.int32, device=net.flat_params.device)
        self._status.view(torch.float32)[1] = 1.0
        self._configure_optim()

    def _zero_frozen_moments(self):
        """Both moments of every frozen slot (`Network.freeze`) to zero: with a zero gradient the update of such a slot is exactly zero."""
        net = self.net
        for p in net._frozen_parameters() if self.frozen[0] else ():
            off, n = net._flat_off[id(p)]
            self.exp_avg[off:off + n].zero_()
            if self.exp_avg_sq is not None:
                self.exp_avg_sq[off:off + n].zero_()

    # ---- AdamW decay / global-norm clipping / weight EMA ----------------------------------------------------------------------
    def _configure_optim(self):
        """Buffers of the options that are on: the decay mask, the partials of the norm, the EMA copy (kept if it already exists)."""
        net = self.net
        if (self.lr_mults is not None or self.optimizer != "adam") and self.group_ids is None:
            # per-stage rates (sd_optim_groups_step): the byte map on the device, the two tables on the host (they travel by value with
            # every launch).  The map carries the decay bit too, so the mask is not built.
            import ctypes as C
            ids, groups = net.optim_groups()
            self.group_ids, self.groups = ids.to(net.flat_params.device), groups
            self._lr_mul = (C.c_float * len(groups))(*(self.lr_mults[stage] if self.lr_mults is not None else 1.0 for stage, _ in groups))
            self._wd_mul = (C.c_float * len(groups))(*(float(decayed) for _, decayed in groups))
        if self.optimizer == "lamb" and self._lamb is None:
            self._lamb = self._build_lamb_table()
        if self.weight_decay > 0 and self.decay_mask is None and self.group_ids is None:
            self.decay_mask = self.build_decay_mask(net)
        if self.clip_grad_norm > 0 and self._partials is None:
            self._partials = torch.empty(L.lib().sd_grad_sumsq_workspace_bytes(net.flat_grads.numel() - self.frozen_off) // 8, dtype=torch.float64,
                                         device=net.flat_params.device)
        if self.ema_decay > 0 and self.ema is None:
            self.ema = net.flat_params.detach().clone()
        if self.ema_decay == 0:
            self.ema = None

    def _build_lamb_table(self):
        """sd_lamb_step's static part: the slot table of the range behind the frozen prefix (`Network.optim_slots()`, shifted by
        `frozen_off`), laid out on the host by sd_lamb_table_build and uploaded once, and the workspace of its per-block partials.
        Returns (table, nslots, nblocks, workspace)."""
        import ctypes as C
        net, lib, off = self.net, L.lib(), self.frozen_off
        slots = [(lo - off, hi - off, adapt) for lo, hi, adapt in net.optim_slots() if lo >= off]
        count, n = len(slots), net.flat_params.numel() - off
        lo = (C.c_int64 * count)(*(s[0] for s in slots))
        hi = (C.c_int64 * count)(*(s[1] for s in slots))
        adapt = (C.c_ubyte * count)(*(int(s[2]) for s in slots))
        need, nblocks = C.c_size_t(), C.c_int()
        L.check(lib.sd_lamb_table_build(lo, hi, adapt, count, n, None, 0, C.byref(need), C.byref(nblocks)), "sd_lamb_table_build")
        host = torch.zeros(need.value // 4, dtype=torch.int32)
        L.check(lib.sd_lamb_table_build(lo, hi, adapt, count, n, host.data_ptr(), need.value, None, None), "sd_lamb_table_build")
        dev = net.flat_params.device
        return host.to(dev), count, nblocks.value, torch.empty(lib.sd_lamb_workspace_bytes(nblocks.value) // 8, dtype=torch.float64, device=dev)

    @staticmethod
    def build_decay_mask(net):
        """One byte per group of four floats of the flat buffer: 1 inside the slots of the 4-D tensors (convolution weights), 0 for
        biases and BatchNorm weight / bias.  Slots are 32-byte aligned and a conv weight has a multiple of four elements, so a group
        never straddles two tensors."""
        mask = torch.zeros(net.flat_params.numel() // 4, dtype=torch.uint8)
        for p in net._flat_order:
            off, n = net._flat_off[id(p)]
            if p.dim() == 4:
                assert off % 4 == 0 and n % 4 == 0, "a convolution weight must fill whole 16-byte groups"
                mask[off // 4:(off + n) // 4] = 1
        return mask.to(net.flat_params.device)

    @staticmethod
    def check_lr_mults(lr_mults):
        """`lr_mults` (None = off, or {stage of OPTIM_STAGES: multiplier}) -> None or the dict over every stage; a stage left out gets 1."""
        if lr_mults is None:
            return None
        from .network import OPTIM_STAGES
        unknown = sorted(set(lr_mults) - set(OPTIM_STAGES))
        if unknown:
            raise ValueError(f"lr_mults: unknown stage(s) {unknown}; the stages are {', '.join(OPTIM_STAGES)}")
        out = {stage: float(lr_mults.get(stage, 1.0)) for stage in OPTIM_STAGES}
        for stage, v in out.items():
            if not 0 <= v < float("inf"):                    # (false for nan)
                raise ValueError(f"lr_mults[{stage!r}] must be finite and >= 0, got {v!r}")
        return out

    @property
    def plain_adam(self):
        return self.weight_decay == 0 and self.clip_grad_norm == 0 and self.ema_decay == 0

    @property
    def grad_norm(self):
        """Global norm of the last step's (averaged) gradient before clipping, as a device tensor; 0 until a step with clipping ran."""
        return self._status.view(torch.float32)[0]

    @property
    def clip_coef(self):
        """Coefficient the last step multiplied its gradient by (1 = not clipped, 0 = step skipped), as a device tensor."""
        return self._status.view(torch.float32)[1]

    @property
    def skipped_steps(self):
        """Steps skipped so far because the gradient norm was not finite, as a device tensor (int32)."""
        return self._status[2]

    def ema_decay_at(self, t):
        """Decay of update number t (1-based): min(ema_decay, (1 + t) / (10 + t)) -- the average follows the weights closely at first."""
        return min(self.ema_decay, (1.0 + t) / (10.0 + t))

    def _optim_step(self, grad_scale):
        """sd_grad_sumsq (only with clipping) + sd_optim_step (with `lr_mults`: sd_optim_groups_step) on the step's stream; nothing is read back."""
        net, lib, st = self.net, L.lib(), L.stream()
        off = self.frozen_off                        # floats; 4 bytes each, one mask byte per four
        n = net.flat_params.numel() - off
        clip = self.clip_grad_norm > 0
        if clip:
            L.check(lib.sd_grad_sumsq(net.flat_grads.data_ptr() + 4 * off, n, self._partials.data_ptr(), self._partials.numel() * 8, st), "sd_grad_sumsq")
        if self.optimizer != "adam":                 # sgd / lamb: always the groups form; the same tail of arguments for both
            tail = (grad_scale, self.weight_decay, self.group_ids.data_ptr() + off // 4, self._lr_mul, self._wd_mul, len(self.groups), self.clip_grad_norm,
                    self._partials.data_ptr() if clip else None, self._partials.numel() if clip else 0,
                    self.ema.data_ptr() + 4 * off if self.ema is not None else None,
                    self.ema_decay_at(self.step_count) if self.ema is not None else 0.0, self._status.data_ptr())
            if self.optimizer == "sgd":
                L.check(lib.sd_sgd_step(net.flat_params.data_ptr() + 4 * off, net.flat_grads.data_ptr() + 4 * off, self.exp_avg.data_ptr() + 4 * off, n,
                                        self.lr, self.momentum, int(self.nesterov), *tail, st), "sd_sgd_step")
                return
            table, nslots, nblocks, ws = self._lamb
            L.check(lib.sd_lamb_step(net.flat_params.data_ptr() + 4 * off, net.flat_grads.data_ptr() + 4 * off, self.exp_avg.data_ptr() + 4 * off,
                                     self.exp_avg_sq.data_ptr() + 4 * off, n, self.step_count, self.lr, self.betas[0], self.betas[1], self.eps, *tail,
                                     table.data_ptr(), nslots, nblocks, ws.data_ptr(), ws.numel() * 8, st), "sd_lamb_step")
            return
        if self.lr_mults is not None:                # per-stage rates: the same single launch, rate and decay looked up per 16-byte group
            L.check(lib.sd_optim_groups_step(net.flat_params.data_ptr() + 4 * off, net.flat_grads.data_ptr() + 4 * off, self.exp_avg.data_ptr() + 4 * off,
                                             self.exp_avg_sq.data_ptr() + 4 * off, n,
                                             self.step_count, self.lr, self.betas[0], self.betas[1], self.eps, grad_scale, self.weight_decay,
                                             self.group_ids.data_ptr() + off // 4, self._lr_mul, self._wd_mul, len(self.groups), self.clip_grad_norm,
                                             self._partials.data_ptr() if clip else None, self._partials.numel() if clip else 0,
                                             self.ema.data_ptr() + 4 * off if self.ema is not None else None,
                                             self.ema_decay_at(self.step_count) if self.ema is not None else 0.0, self._status.data_ptr(), st),
                    "sd_optim_groups_step")
            return
        L.check(lib.sd_optim_step(net.flat_params.data_ptr() + 4 * off, net.flat_grads.data_ptr() + 4 * off, self.exp_avg.data_ptr() + 4 * off,
                                  self.exp_avg_sq.data_ptr() + 4 * off, n,
                                  self.step_count, self.lr, self.betas[0], self.betas[1], self.eps, grad_scale, self.weight_decay,
                                  self.decay_mask.data_ptr() + off // 4 if self.decay_mask is not None else None, self.clip_grad_norm,
                                  self._partials.data_ptr() if clip else None, self._partials.numel() if clip else 0,
                                  self.ema.data_ptr() + 4 * off if self.ema is not None else None,
                                  self.ema_decay_at(self.step_count) if self.ema is not None else 0.0, self._status.data_ptr(), st), "sd_optim_step")

    @contextmanager
    def ema_weights(self):
        """Run the body on the averaged weights: the contents of `flat_params` and the EMA buffer are exchanged on entry and exchanged
        back, bit for bit, on exit (every parameter of the network is a view of `flat_params`).  BatchNorm running statistics are
        shared, not averaged.  Without an EMA (`ema_decay == 0`) the body runs on the weights as they are."""
        if self.ema is None:
            yield
            return
        self._swap_ema()
        try:
            yield
        finally:
            self._swap_ema()

    def _swap_ema(self):
        with torch.no_grad():
            held = self.net.flat_params.clone()
            self.net.flat_params.copy_(self.ema)
            self.ema.copy_(held)
        self.net.invalidate_folded()                 # the eval forward caches folded BatchNorm affines and bf16 weight copies

    # ---- true resume: the reference saves weights only (trainer.py:226-237), so a run cannot continue --------
    def state_dict(self):
        """Optimizer state of the flat-buffer Adam: both moment buffers, the step count (bias correction) and the learning rate.
        Tensors are copies on the host; `Network.state_dict()` carries the weights and BatchNorm buffers."""
        state = {"exp_avg": self.exp_avg.detach().cpu().clone(), "exp_avg_sq": None if self.exp_avg_sq is None else self.exp_avg_sq.detach().cpu().clone(),
                 "step_count": int(self.step_count), "lr": float(self.lr), "betas": tuple(self.betas), "eps": float(self.eps),
                 "flat_numel": int(self.net.flat_params.numel())}
        if not self.plain_adam:          # (one host read of the skip counter: state_dict is a checkpoint, not the step)
            state.update(weight_decay=self.weight_decay, clip_grad_norm=self.clip_grad_norm, ema_decay=self.ema_decay,
                         skipped_steps=int(self.skipped_steps), ema=None if self.ema is None else self.ema.detach().cpu().clone())
        if self.optimizer != "adam":     # (a state without the key is Adam's: files from before the choice existed)
            state.update(optimizer=self.optimizer, momentum=self.momentum, nesterov=self.nesterov)
            if self.exp_avg_sq is None:
                del state["exp_avg_sq"]
        return state

    def load_state_dict(self, state):
        if int(state["flat_numel"]) != self.net.flat_params.numel():
            raise L.SdError(f"optimizer state is for a flat parameter buffer of {state['flat_numel']} floats, this network has "
                            f"{self.net.flat_params.numel()} (different labels / parts / fpn_depth?)")
        kind = state.get("optimizer", "adam")
        if kind != self.optimizer:
            raise L.SdError(f"optimizer state was written by optimizer {kind!r}, this step was built with optimizer {self.optimizer!r}: the moment "
                            "buffers of one rule mean nothing to another (resume with the run's --optimizer, or start from the weights alone)")
        self.exp_avg.copy_(state["exp_avg"])
        if self.exp_avg_sq is not None:
            self.exp_avg_sq.copy_(state["exp_avg_sq"])
        if kind == "sgd":                            # the momentum travels with the run, like the options below
            self.momentum, self.nesterov = float(state.get("momentum", self.momentum)), bool(state.get("nesterov", self.nesterov))
        self.step_count, self.lr = int(state["step_count"]), float(state["lr"])
        self.betas, self.eps = tuple(state["betas"]), float(state["eps"])
        # the options travel with the run; a file written without them (or before they existed) loads with all three off
        self.weight_decay, self.clip_grad_norm = float(state.get("weight_decay", 0.0)), float(state.get("clip_grad_norm", 0.0))
        self.ema_decay = float(state.get("ema_decay", 0.0))
        self._configure_optim()
        if self.ema is not None:
            self.ema.copy_(state["ema"] if state.get("ema") is not None else self.net.flat_params)
        self._status[2] = int(state.get("skipped_steps", 0))
        self._zero_frozen_moments()                  # (a state written under another freeze setting may hold moments for slots frozen now)

    def sync_parameters(self):
        """Identical initial weights on every rank (rank 0's)."""
        if self.world > 1:
            dist.broadcast(self.net.flat_params, 0, group=self.pg)
            for b in self.net.buffers():
                dist.broadcast(b, 0, group=self.pg)
            if self.ema is not None and self.step_count == 0:       # the average starts from the weights every rank now holds
                self.ema.copy_(self.net.flat_params)

    # Bucket plans: which stages travel together.  A group is launched when its LAST stage completes; the stages of a group are adjacent in
    # the flat buffer (parameters are laid out in registration order: stem, down1 .. down4, FPN, head -- the backward completes them from
    # the end), so a group is ONE contiguous all-reduce.  Five launches hide best under a 73 ms fp32 step; a 15 ms mixed-precision step pays
    # ~0.08 ms of fixed cost per launch (stream hand-offs on both sides + the launch itself: `profiles/r05_comm_sim_sweep.txt`).
    BUCKET_PLANS = {5: (("fpn_head",), ("down4",), ("down3",), ("down2",), ("down1_stem",)),
                    3: (("fpn_head", "down4"), ("down3",), ("down2", "down1_stem")),
                    2: (("fpn_head", "down4", "down3"), ("down2", "down1_stem")),
                    1: (("fpn_head", "down4", "down3", "down2", "down1_stem"),)}

    def set_bucket_plan(self, launches):
        """Number of all-reduce launches per step: 5 (default: one per parameter group), 3, 2 or 1."""
        if launches not in self.BUCKET_PLANS:
            raise ValueError(f"bucket plan must be one of {sorted(self.BUCKET_PLANS)}, got {launches!r}")
        self.bucket_plan = launches

    def _groups(self):
        """{trigger stage: (lo, hi)} of the current plan: the flat range a group covers, keyed by the stage that completes it."""
        out = {}
        for group in self.BUCKET_PLANS[getattr(self, "bucket_plan", 5)]:
            lo = min(self.ranges[n][0] for n in group); hi = max(self.ranges[n][1] for n in group)
            assert hi - lo == sum(self.ranges[n][1] - self.ranges[n][0] for n in group), "the stages of a bucket group must be adjacent in the flat buffer"
            out[group[-1]] = (lo, hi)
        return out

    def _exchange_hooks(self):
        """(on_stage, finish): on_stage(name) starts the all-reduce of the gradient bucket group that stage `name` completes (called by the
        backward schedule as soon as that parameter group's gradients are complete), finish() joins every launch before the Adam launch."""
        net = self.net
        groups = self._groups()
        sim = getattr(self, "sim", None)
        if sim is not None and self.exchange_enabled:
            return (lambda name: sim.all_reduce(net.flat_grads, *groups[name]) if name in groups else None), sim.wait
        if self.world == 1 or not self.exchange_enabled:
            return None, (lambda: None)
        if self.rccl is not None:
            return (lambda name: self.rccl.all_reduce(net.flat_grads, *groups[name]) if name in groups else None), self.rccl.wait
        works = []

        def on_stage(name):
            if name in groups:
                lo, hi = groups[name]
                works.append(dist.all_reduce(net.flat_grads[lo:hi], group=self.pg, async_op=True))

        def finish():
            for w in works:
                w.wait()
        return on_stage, finish

    STAGES = ("fpn_head", "down4", "down3", "down2", "down1_stem")       # order in which the backward completes the buckets

    def attach_sim(self, ranks=8, workgroups=32, gbps=200.0):
        """Run every following step with the simulated exchange (`SimExchange`) beside its backward; `detach_sim()` ends it."""
        if self.world > 1:
            raise L.SdError("attach_sim replaces the gradient exchange by a stand-in that moves no gradients: single-rank sizing runs only "
                            f"(this step has {self.world} ranks)")
        # (scratch as large as the whole flat buffer: a bucket plan may send several parameter groups -- up to all of them -- in one launch)
        self.sim = SimExchange(self.net.flat_params.device, int(self.net.flat_grads.numel()), ranks, workgroups, gbps)
        return self.sim

    def detach_sim(self):
        self.sim = None

    def verify_exchange(self):
        """Self-check of the data-parallel exchange THROUGH THE PATH THE STEP USES (same buckets, same binding, same streams):
        every rank fills its flat gradient buffer with rank+1, the five buckets are summed, and every element must read
        world*(world+1)/2 on every rank.  Returns the report bench.py prints; raises if a rank is missing from the sum."""
        net, n = self.net, self.world
        report = {"ranks": n, "exchange": self.exchange_name(), "buckets": {k: self.ranges[k][1] - self.ranges[k][0] for k in self.STAGES}}
        if n == 1:
            report["check"] = "single rank: no exchange"
            return report
        rank = dist.get_rank(self.pg)
        net.flat_grads.fill_(float(rank + 1))
        on_stage, finish = self._exchange_hooks()
        for name in self.STAGES:
            on_stage(name)
        finish()
        want = n * (n + 1) / 2
        lo, hi = float(net.flat_grads.min()), float(net.flat_grads.max())
        net.flat_grads.zero_()
        if lo != want or hi != want:
            raise L.SdError(f"gradient exchange check failed on rank {rank}: sum of (rank+1) over {n} ranks should be {want}, got [{lo}, {hi}]")
        report["check"] = f"ok: sum(rank+1) == {want:g} in all {len(self.STAGES)} buckets on every rank"
        return report

    def exchange_name(self):
        if self.world == 1:
            return "none"
        if self.rccl is not None:
            return "sd_allreduce (RCCL via C ABI)"
        return f"torch.distributed {dist.get_backend(self.pg)}"

    def time_buckets(self, iters=5):
        """Isolated duration of each bucket's all-reduce in microseconds (stream events around a blocking all-reduce of the
        bucket, nothing else running; median of `iters`): what the overlap with the backward kernels has to hide."""
        if self.world == 1:
            return {}
        net, out = self.net, {}
        for name in self.STAGES:
            lo, hi = self.ranges[name]
            ts = []
            for _ in range(iters + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if self.rccl is not None:
                    self.rccl.all_reduce(net.flat_grads, lo, hi); self.rccl.wait()
                else:
                    dist.all_reduce(net.flat_grads[lo:hi], group=self.pg)
                e1.record(); e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            ts = sorted(ts[1:])
            out[name] = {"floats": hi - lo, "us": round(ts[len(ts) // 2], 1),
                         "algbw_GBps": round((hi - lo) * 4 / (ts[len(ts) // 2] * 1e-6) / 1e9, 1)}
        net.flat_grads.zero_()
        return out

    def _accumulate(self, dst, src, name, overwrite):
        """One `sd_grad_accum` launch over stage `name`'s range behind the frozen prefix, on the step's stream: dst (+)= src."""
        lo, hi = self.ranges[name]
        lo = max(lo, self.frozen_off)
        if hi <= lo:                                     # a stage that is frozen whole: nothing of it is read or written
            return
        T.push("accum:" + name)
        L.check(L.lib().sd_grad_accum(dst.data_ptr() + 4 * lo, src.data_ptr() + 4 * lo, hi - lo, int(overwrite), L.stream()), "sd_grad_accum")
        T.pop()

    def _accum_hook(self, exchange, last):
        """on_stage of a micro-step under accumulation.  Not the last of its group: the stage's gradient goes into `grad_acc` (the first
        micro-step overwrites, so the buffer is never zero-filled) and nothing else runs.  The last: `grad_acc` is added into
        `flat_grads`, then the stage's exchange hook (if there is an exchange) starts -- every exchange orders its own stream behind
        the stream this launch is on (torch's binding and both side-stream exchanges wait for the current stream when they are
        called), so the all-reduce reads the total."""
        net, acc, first = self.net, self.grad_acc, self.micro == 0

        def on_stage(name):
            if not last:
                self._accumulate(acc, net.flat_grads, name, first)
                return
            self._accumulate(net.flat_grads, acc, name, False)
            if exchange is not None:
                exchange(name)
        return on_stage

    def _update(self, k):
        """The optimizer launch on `flat_grads` = the sum over k micro-batches (and, after the exchange, over the ranks): one more
        optimizer step, on the mean."""
        net = self.net
        grad_scale = 1.0 / (k * self.world)
        self.step_count += 1
        T.push("adam")
        if self.plain_adam and self.lr_mults is None and self.optimizer == "adam":
            off = 4 * self.frozen_off                # bytes: the frozen stages' prefix is not the optimizer's
            L.check(L.lib().sd_adam_step(net.flat_params.data_ptr() + off, net.flat_grads.data_ptr() + off, self.exp_avg.data_ptr() + off,
                                         self.exp_avg_sq.data_ptr() + off, net.flat_params.numel() - self.frozen_off, self.step_count, self.lr, self.betas[0],
                                         self.betas[1], self.eps, grad_scale, L.stream()), "sd_adam_step")
        else:
            self._optim_step(grad_scale)
        T.pop()

    def __call__(self, images, targets):
        """One batch in, that batch's loss vector [total, hm, offset, embedding] out, as a device tensor.  Without accumulation this is
        one optimizer step; with `accum_steps` = K it is one micro-step, and every K-th call runs the optimizer (`self.updated`)."""
        net = self.net
        accumulate = self.accum_steps > 1
        last = self.micro + 1 >= self.accum_steps                  # this call completes its group (always, without accumulation)
        T.push("step" if last else "accum")
        T.push("forward")
        if self.bn_sync is None:
            head, tape = net.forward_train(images, amp=self.amp)
        else:
            head, tape = net.forward_train(images, amp=self.amp, bn_sync=self.bn_sync)
        T.pop()
        T.push("loss")
        M, N = net.label_count, net.part_count
        cfg = loss_config(self.args, M, N, targets["anchor_inds"].shape[1], targets["part_inds"].shape[1])
        desc, keep, out8 = loss_forward(head, targets, cfg)
        dhead = loss_backward(desc, out8, self.one, tuple(head.shape))
        T.pop()
        on_stage, finish = self._exchange_hooks() if last else (None, None)      # gradients travel once per optimizer step
        if on_stage is not None and T.enabled():
            launch = on_stage

            def on_stage(name):                                    # every gradient bucket as its own range
                T.push("bucket:" + name)
                launch(name)
                T.pop()
        if accumulate:
            on_stage = self._accum_hook(on_stage, last)
        T.push("backward")
        net.backward_from(tape, dhead, on_stage)
        T.pop()
        self.micro += 1
        if last:
            T.push("exchange:join")
            finish()
            T.pop()
            self._update(self.micro)
            self.micro = 0
        self.updated = last
        T.pop()
        self.stats.update(out8[1], out8[2], out8[3])
        return out8[:4]

    def flush(self):
        """Ends a partial group (0 < `micro` < K: the batches of an epoch ran out) with what it holds: `flat_grads` takes the sum from
        `grad_acc`, the gradients are exchanged and the optimizer runs on the mean over `micro` micro-batches.  Nothing happens, and
        nothing is launched, at `micro` == 0.  Under data parallelism every rank must call it at the same point (it exchanges).
        Returns whether an optimizer step ran."""
        if self.micro == 0:
            return False
        T.push("step")
        on_stage, finish = self._exchange_hooks()
        for name in self.STAGES:                                   # the order in which a backward would have completed them
            self._accumulate(self.net.flat_grads, self.grad_acc, name, True)
            if on_stage is not None:
                on_stage(name)
        T.push("exchange:join")
        finish()
        T.pop()
        self._update(self.micro)
        self.micro = 0
        self.updated = True
        T.pop()
        return True


def train_step_kwargs(args):
    """Keyword arguments `Trainer` builds its `TrainStep` with from the parsed command line."""
    kw = dict(lr=args.learning_rate, sync_bn=bool(getattr(args, "sync_bn", False)))
    for name in ("weight_decay", "clip_grad_norm", "ema_decay"):          # optimizer options: passed when set (TrainStep's defaults are "off")
        if getattr(args, name, 0.0):
            kw[name] = float(getattr(args, name))
    from ..utils.args import check_accum, check_lr, check_optimizer, stage_lr_mults
    kind = check_optimizer(args)                                          # --optimizer / --momentum / --nesterov: passed when not adam
    if kind.optimizer != "adam":
        kw.update(optimizer=kind.optimizer, momentum=kind.momentum, nesterov=kind.nesterov)
    lr = check_lr(args)
    mults = stage_lr_mults(lr.backbone_lr_mult, lr.lr_layer_decay)        # --backbone_lr_mult / --lr_layer_decay: None when both are 1
    if mults is not None:
        kw["lr_mults"] = mults
    accum = check_accum(args)                                             # --accum_steps: passed when > 1
    if accum > 1:
        kw["accum_steps"] = accum
    return kw


class LRSchedule:
    """The scalar learning rate of every optimizer step, written to `TrainStep.lr` (a kernel argument: nothing synchronises).
    schedule "step": torch.optim.lr_scheduler.StepLR(step_size, gamma=0.1) over the epochs (trainer.py:54-56),
    base * gamma ** (epoch // step_size), moved by `step()` once per epoch.  "cosine": with i = `TrainStep.step_count` before the step,
    N = warmup_steps, T = total_steps: min_lr + (base - min_lr) * 0.5 * (1 + cos(pi * (i - N) / (T - N))) for N <= i < T, min_lr from T on.
    Warm-up, either schedule: the value is multiplied by (i + 1) / N while i < N (the cosine term is `base` there).  Python floats.
    Without warm-up and with "step" (`per_step` False) the rate changes in `step()` only, to StepLR's values, bit for bit; otherwise the
    loop calls `apply()` before every optimizer step.  The curve is a function of `step_count`, which the optimizer state carries: a
    resumed run continues on it."""

    NEW_KEYS = ("schedule", "warmup_steps", "total_steps", "min_lr")

    def __init__(self, step: TrainStep, step_size: int, gamma: float = 0.1, schedule: str = "step", warmup_steps: int = 0, total_steps: int = 0,
                 min_lr: float = 0.0):
        self.step_obj, self.step_size, self.gamma, self.epoch, self.base = step, max(int(step_size), 1), gamma, 0, step.lr
        if schedule not in ("step", "cosine"):
            raise ValueError(f"schedule must be 'step' or 'cosine', got {schedule!r}")
        self.schedule, self.warmup_steps, self.total_steps, self.min_lr = schedule, int(warmup_steps), int(total_steps), float(min_lr)
        if self.per_step and not 0 <= self.warmup_steps < self.total_steps:
            raise ValueError(f"the warm-up ({self.warmup_steps} steps) must be shorter than the run ({self.total_steps} optimizer steps)")

    @property
    def per_step(self):
        return self.schedule != "step" or self.warmup_steps > 0

    def lr_at(self, i):
        """The rate of the optimizer step that finds `step_count` == i."""
        import math
        n, t = self.warmup_steps, self.total_steps
        if self.schedule == "step":
            value = self.base * self.gamma ** (self.epoch // self.step_size)
        elif i < n:
            value = self.base
        elif i < t:
            value = self.min_lr + (self.base - self.min_lr) * 0.5 * (1 + math.cos(math.pi * (i - n) / (t - n)))
        else:
            value = self.min_lr
        return value * ((i + 1) / n) if i < n else value

    def _set(self):
        # (per epoch the step schedule needs the epoch alone: `step_count` is read only where a per-step schedule is on)
        self.step_obj.lr = self.lr_at(self.step_obj.step_count if self.per_step else 0)

    def apply(self):
        """Before an optimizer step: its rate into `TrainStep.lr`; returns it."""
        self.step_obj.lr = self.lr_at(self.step_obj.step_count)
        return self.step_obj.lr

    def step(self):
        self.epoch += 1
        self._set()

    def describe(self):
        text = f"StepLR every {self.step_size} epoch(s)" if self.schedule == "step" else \
            f"cosine from {self.base:g} to {self.min_lr:g} over {self.total_steps} optimizer steps"
        return text + (f", linear warm-up over the first {self.warmup_steps} steps" if self.warmup_steps else "")

    def state_dict(self):
        return {"epoch": self.epoch, "base": self.base, "step_size": self.step_size, "gamma": self.gamma, "schedule": self.schedule,
                "warmup_steps": self.warmup_steps, "total_steps": self.total_steps, "min_lr": self.min_lr}

    def load_state_dict(self, state):
        """A state from before the schedule options (today's four keys) stands for schedule "step" without warm-up.  The options belong
        to the command line AND to the curve a run is on: a state whose schedule, warm-up, total or min_lr differ from this object's is
        refused (the total only where a per-step schedule uses it)."""
        was = (state.get("schedule", "step"), int(state.get("warmup_steps", 0)), float(state.get("min_lr", 0.0)))
        now = (self.schedule, self.warmup_steps, self.min_lr)
        total = int(state.get("total_steps", self.total_steps))
        if was != now or (self.per_step and total != self.total_steps):
            raise ValueError("resume: the checkpoint was written with --lr_schedule %s --warmup_steps %d --min_lr %g over %d optimizer steps, the "
                             "command line gives --lr_schedule %s --warmup_steps %d --min_lr %g over %d: continue with the checkpoint's values "
                             "(same --epochs / --steps / --batch_size)" % (was + (total,) + now + (self.total_steps,)))
        self.epoch, self.base, self.step_size, self.gamma = int(state["epoch"]), float(state["base"]), int(state["step_size"]), float(state["gamma"])
        self._set()


StepLR = LRSchedule          # (the name this class had while it held the step schedule only)


def shard_indices(n, batch, rank, world, seed):
    """Per-rank batches of sample indices for one epoch of data-parallel training over a real dataset.
    Every rank draws the SAME permutation (shared seed = base seed + epoch), truncates it to whole global batches
    (drop_last=True, trainer.py:69, applied to the global batch `batch * world`) and takes the strided shard
    `[rank::world]`: shards are disjoint, cover the truncated permutation and have the same number of steps on every
    rank, so the bucketed all-reduces of all ranks pair up step by step."""
    import numpy as np
    order = np.random.default_rng(seed).permutation(n)
    usable = (n // (batch * world)) * batch * world
    mine = order[:usable][rank::world]
    return [mine[i:i + batch] for i in range(0, len(mine), batch)]


class Trainer:
    """Epoch loop around TrainStep with the reference's knobs (src/sdnet/model/trainer.py:23-237): Adam(lr),
    StepLR(step_size=args.lr_step), validation every second epoch with the Decoder + Evaluator + Loss and the four
    `model_best_{loss,csi,classif,kp_reg}.pth` checkpoints in trainings/<timestamp>/.  Data: a directory of JSON+image
    samples (no augmentation) or `--synthetic N` seeded scenes rendered on the GPU.  `--train_tiles` trains on windows of the directory's
    images at the tile scale of `evaluate --tiles`; the validation pass here always shows whole frames.  TensorBoard logging and the PIL
    augmentations are outside the hot path."""

    def __init__(self, args):
        from datetime import datetime
        from pathlib import Path

        import numpy as np

        from ..data import CropDataset, Encode
        from ..utils.args import check_freeze, check_lr, check_train
        from .network import Network
        self.args = args
        check_train(args)                                              # --train_tiles, --keep_aspect, --aug_*: ranges, square inputs, --synthetic
        self.freeze = check_freeze(args)                               # --freeze_stages N, --freeze_bn
        self.lr_options = check_lr(args)                               # --lr_schedule, --warmup_steps, --min_lr, --backbone_lr_mult, --lr_layer_decay
        if getattr(args, "use_amp", False) and not BF16_TRAINING:
            # the reference autocasts the training forward under --amp (trainer.py:115-121); silently training in fp32 under the
            # same flag would be a different experiment with the same name
            raise NotImplementedError("--amp: the bf16 training step is not built; train without --amp (fp32), or use "
                                      "--bf16_inference to run only the validation / inference forward on the bf16 backbone")
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.epoch = 0
        self.net = Network(args, pretrained=True)
        if args.pretrained_model:
            self.net.load_state_dict(torch.load(args.pretrained_model, map_location="cpu", weights_only=True))
        self.net.to(args.device).train()
        self.net.freeze(*self.freeze)                                  # before the step is built: TrainStep reads the setting
        self.step = TrainStep(self.net, args, **train_step_kwargs(args))
        self.step.sync_parameters()
        self.encode = Encode(args)
        self.rng = np.random.default_rng(926354916 + self.rank)
        # directory data: decode on the host (PIL), resize + flips + normalisation for the whole batch on the GPU
        from ..data.augment import TrainAugmentation
        self.dataset = None if args.synthetic else CropDataset(args, args.train_dir, raw=True)
        # --lr_schedule / --warmup_steps / --min_lr over the optimizer steps of the run: epochs x steps per epoch of this world size, as
        # `batches()` counts them, or --steps when that is set and smaller
        lr = self.lr_options
        from ..utils.args import run_updates
        total = run_updates(args.epochs, self.batches_per_epoch(), self.step.accum_steps, args.steps)
        if (lr.schedule != "step" or lr.warmup_steps) and lr.warmup_steps >= total:
            raise ValueError(f"'warmup_steps' ({lr.warmup_steps}) should be less than the optimizer steps of the run ({total}: --epochs x steps per "
                             "epoch, or --steps)")
        self.scheduler = LRSchedule(self.step, args.lr_step, schedule=lr.schedule, warmup_steps=lr.warmup_steps, total_steps=total, min_lr=lr.min_lr)
        self.augment = TrainAugmentation(args)
        self.save_dir = Path("trainings") / f"{datetime.now():%Y-%m-%d_%H-%M-%S}"
        self.best_loss = float("inf")
        self.best_csi = self.best_classif = self.best_kp_reg = 0.0
        from ..data import Decoder
        from .evaluator import Evaluator
        from .loss import Loss
        self.decoder, self.evaluator, self.loss = Decoder(args), Evaluator(args), Loss(args)
        self.valid_set = None if args.synthetic or not args.valid_dir else CropDataset(args, args.valid_dir, raw=True)
        # --cache_images GB: decoded images kept in device memory across epochs, one cache for both sets, filled before epoch 1
        from ..data.image_cache import from_args
        self.cache = None if args.synthetic else from_args(args)
        self.start_epoch = 0
        self.global_step = 0                      # trainer.py:35,129: images seen, the x axis of every scalar
        self._writer = None
        if getattr(args, "resume", None):
            self.load_resume(args.resume)

    def batches_per_epoch(self):
        """Batches of one epoch on this world size, as `batches()` yields them (whole global batches: drop_last)."""
        a, world = self.args, self.step.world
        if a.synthetic:
            return max(a.synthetic // (a.batch_size * world), 1)
        return len(self.dataset) // (a.batch_size * world)

    def steps_per_epoch(self):
        """Optimizer steps of one epoch: its batches, or with `--accum_steps K` ceil(batches / K) (the last group is flushed)."""
        from ..utils.args import updates_per_epoch
        return updates_per_epoch(self.batches_per_epoch(), self.step.accum_steps)

    def batches(self):
        a, B = self.args, self.args.batch_size
        world = self.step.world
        if a.synthetic:
            from ..data.synthetic import synthetic_batch
            gen = torch.Generator(device=a.device).manual_seed(926354916 + self.rank)
            for _ in range(max(a.synthetic // (B * world), 1)):
                flat = synthetic_batch(self.rng, B, a.width, a.height, len(a.labels), len(a.parts))
                images = torch.randn(B, 3, a.height, a.width, device=a.device, generator=gen)
                yield images, self.encode.render(self.encode.plan(a.width, a.height, *flat), a.device)
        else:
            # decode threads + pinned staging + side-stream upload, `prefetch` batches ahead of the step (data/feeder.py); resize, jitter,
            # flips, normalisation and the targets for the whole batch on the GPU (the reference: trainer.py:62-72, dataset.py:41-49)
            from ..data.feeder import BatchFeeder, default_decode_workers
            shards = shard_indices(len(self.dataset), B, self.rank, world, 926354916 + self.epoch)
            workers = getattr(a, "decode_workers", 0) or default_decode_workers(world)
            # While the feed runs, torch's intra-op pool is single-threaded: the loop's host work is thousands of tiny tensor ops and kernel
            # launches, the pool gives them nothing and its workers spin against the decode threads (measured: 64 x 7 scalar draws 450 ms
            # next to 16 decoders, 7 ms alone).  The reference's DataLoader workers run single-threaded for the same reason.
            threads = torch.get_num_threads()
            torch.set_num_threads(1)
            try:
                for batch in BatchFeeder(self.dataset, shards, a.device, workers=workers, depth=getattr(a, "prefetch", 3), cache=self.cache):
                    images, anns = self.augment(batch, batch.annotations)
                    yield images, self.encode.batch(self.augment.size, anns, a.device)
            finally:
                torch.set_num_threads(threads)

    def valid_batches(self):
        """Per batch of this rank's contiguous shard of the validation set, in order: (predictions, annotations in network-input pixels,
        raw_parts, the batch's head views).  Directory: `--eval_batch` images per forward + decoder launch (model/predictor.py);
        synthetic: one forward per image, as always, grouped `--eval_batch` at a time for the loss."""
        from itertools import islice

        from ..utils.distributed import shard_range
        a, world = self.args, self.step.world
        if self.valid_set is not None:
            # decode threads -> GPU Resize + Normalize -> forward + decoder at --eval_batch images per launch (model/predictor.py)
            from .predictor import batched_decodes
            yield from batched_decodes(self.net, self.decoder, self.valid_set, a, cache=self.cache,
                                       index_range=shard_range(len(self.valid_set), self.rank, world))
            return
        from ..data.synthetic import synthetic_samples
        n = min(max(a.synthetic, 1), 16)
        lo, hi = shard_range(n, self.rank, world)
        batch = int(getattr(a, "eval_batch", 16) or 16)
        group = []

        def collate(group):
            preds, anns, raws, outs = zip(*group)
            return list(preds), list(anns), list(raws), {k: torch.cat([o[k] for o in outs]) for k in outs[0]}

        for image, annotation in islice(synthetic_samples(a, n, seed=20261003), lo, hi):
            with torch.no_grad():
                output = self.net(image[None].to(a.device))
                data = self.decoder(output, return_metadata=True, metadata_fields=("annotation", "raw_parts"))
            group.append((data["annotation"][0], annotation, data["raw_parts"][0], output))
            if len(group) == batch:
                yield collate(group)
                group = []
        if group:
            yield collate(group)

    def _take_rank0_buffers(self):
        """Data-parallel validation scores rank 0's model (the one reported and saved): every rank keeps a copy of its own BatchNorm
        running statistics (rank-local unless the step runs synchronized BatchNorm) and takes rank 0's by broadcast.  Returns the copies for `_restore_buffers`."""
        own = [b.detach().clone() for b in self.net.buffers()]
        for b in self.net.buffers():
            dist.broadcast(b, 0, group=self.step.pg)
        self.net.invalidate_folded()                                 # the eval forward caches folded BatchNorm affines
        return own

    def _restore_buffers(self, own):
        with torch.no_grad():
            for b, o in zip(self.net.buffers(), own):
                b.copy_(o)
        self.net.invalidate_folded()

    def valid(self):
        """Validation pass of the reference (src/sdnet/model/trainer.py:137-237): eval-mode forward, Decoder + Evaluator + Loss PER IMAGE
        (the loss statistics are means over images of per-image losses, :160-168), then the four `model_best_*.pth` checkpoints
        (rank 0 only).  Forward and decoder run batched; the per-image losses of a batch come from one Encode and one
        `Loss.per_image` launch pair (bit-identical to one loss call per image).
        Data-parallel: each rank runs its contiguous shard (utils/distributed.py) with rank 0's BatchNorm buffers; per-image loss rows
        and Evaluators are gathered in rank order, so every rank returns the stats of one pass over the whole set in sample order
        and keeps the same best-so-far values; afterwards each rank has its own buffers back.
        With `--ema_decay` the pass, the best-model selection and the `model_best_*.pth` files use the averaged weights
        (`TrainStep.ema_weights()`); the raw weights are back in place when it returns."""
        with self.step.ema_weights():
            return self._valid()

    def _valid(self):
        from ..utils.distributed import gather_evaluator, gather_rows
        a = self.args
        world = self.step.world
        own = self._take_rank0_buffers() if world > 1 else None
        self.net.eval()
        self.evaluator.reset()
        rows = []
        try:
            for predictions, annotations, raw_parts, output in self.valid_batches():
                with torch.no_grad():
                    # the Evaluator sees each annotation before Encode clips it in place, as in the reference's per-image loop
                    self.evaluator.accumulate_batch(predictions, annotations, raw_parts, eval_csi=True, eval_classif=True)
                    # the annotations are in network-input pixels (resized + clipped / the synthetic generator): encode them as the targets
                    target = self.encode.batch((a.width, a.height), annotations, a.device)
                    rows.append(self.loss.per_image(output, target)[:, 1:4])         # hm, offset, embedding per image
        finally:
            if own is not None:
                self._restore_buffers(own)
            self.net.train()
        rows = torch.cat(rows) if rows else torch.zeros((0, 3), dtype=torch.float32, device=a.device)
        rows = gather_rows(rows, self.step.pg)                     # every image of the set, in sample order
        self.evaluator = gather_evaluator(self.evaluator, self.step.pg)
        n = rows.shape[0]
        stats = LossStats()
        if n:                                                      # one host sync for the whole pass
            stats = LossStats(*(rows.double().sum(0).tolist()))
            stats /= n
        f1_csi = self.evaluator.csi_eval.reduce().f1_score
        f1_classif = self.evaluator.classification_eval.reduce().f1_score
        f1_kp = self.evaluator.kps_eval.reduce().f1_score
        if self.rank == 0:
            self.save_dir.mkdir(parents=True, exist_ok=True)
            from ..utils.scalars import metric_dicts
            writer = self.scalar_writer()
            writer.add_scalars("Loss/Validation", dict(hm_loss=stats.hm_loss, offset_loss=stats.offset_loss,
                                                        embedding_loss=stats.embedding_loss), self.global_step)      # trainer.py:240-242
            for tag, values in metric_dicts(self.evaluator).items():                                                 # trainer.py:243-256
                writer.add_scalars(tag, values, self.global_step)
            writer.flush()
            print(f"validation ({n} images): loss {stats.total_loss:.5f} | kp F1 {f1_kp:.2%} | CSI F1 {f1_csi:.2%} | classification F1 {f1_classif:.2%}", flush=True)
        for value, attr, name, better in ((stats.total_loss, "best_loss", "loss", lambda v, b: v < b), (f1_csi, "best_csi", "csi", lambda v, b: v > b),
                                          (f1_classif, "best_classif", "classif", lambda v, b: v > b), (f1_kp, "best_kp_reg", "kp_reg", lambda v, b: v > b)):
            if better(value, getattr(self, attr)):
                setattr(self, attr, value)                         # on every rank: all ranks see the same merged numbers
                if self.rank == 0:
                    self.net.save(self.save_dir / f"model_best_{name}.pth")
        return stats

    # ---- true resume: weights + BatchNorm buffers + Adam moments / step + StepLR epoch + best-so-far metrics + epoch counter ----
    def save_resume(self, path):
        """Everything the next epoch depends on: weights + BatchNorm buffers, Adam moments / step / lr, StepLR epoch, best-so-far
        metrics, the multi-scale input size drawn for the next epoch (trainer.py:135), the random streams the augmentation and the
        synthetic scenes draw from (torch's global generator, this rank's numpy generator) and the run's save directory -- tensors
        and plain Python values only, so that the file loads with `weights_only=True`."""
        torch.save({"model": {k: v.detach().cpu().clone() for k, v in self.net.state_dict().items()},
                    "optimizer": self.step.state_dict(), "scheduler": self.scheduler.state_dict(), "epoch": self.epoch,
                    "best": {k: getattr(self, k) for k in ("best_loss", "best_csi", "best_classif", "best_kp_reg")},
                    "augment_size": tuple(int(v) for v in self.augment.size), "torch_rng": torch.get_rng_state(),
                    "numpy_rng": self.rng.bit_generator.state, "save_dir": str(self.save_dir), "global_step": int(self.global_step),
                    "freeze_stages": int(self.freeze[0]), "freeze_bn": bool(self.freeze[1]),
                    "lr_mults": None if self.step.lr_mults is None else dict(self.step.lr_mults)}, path)

    def load_resume(self, path):
        from pathlib import Path
        state = torch.load(path, map_location="cpu", weights_only=True)
        self.net.load_state_dict(state["model"])
        asked = (self.step.weight_decay, self.step.clip_grad_norm, self.step.ema_decay)
        self.step.load_state_dict(state["optimizer"])
        kept = (self.step.weight_decay, self.step.clip_grad_norm, self.step.ema_decay)
        if kept != asked and self.rank == 0:            # the options belong to the run: the file's win over the command line's, and say so
            print("resume: optimizer options come from the checkpoint -- weight_decay %g, clip_grad_norm %g, ema_decay %g (the command line "
                  "asked for %g, %g, %g); a checkpoint written without them continues with all three off" % (kept + asked), flush=True)
        was, now = state.get("lr_mults"), self.step.lr_mults
        if was != now and self.rank == 0:               # the per-stage multipliers belong to the command line too, as the freeze does
            def show(mults):
                return "none" if mults is None else ", ".join(f"{stage} {v:g}" for stage, v in mults.items())
            print(f"resume: the checkpoint was written with the per-stage learning-rate multipliers {show(was)}, this run continues with "
                  f"{show(now)} (--backbone_lr_mult / --lr_layer_decay: the command line wins)", flush=True)
        self.scheduler.load_state_dict(state["scheduler"])
        self.start_epoch = int(state["epoch"]) + 1
        for k, v in state["best"].items():
            setattr(self, k, v)
        if "augment_size" in state:                     # (files written before round 3 carry the weights / optimizer part only)
            self.augment.size = tuple(int(v) for v in state["augment_size"])
            torch.set_rng_state(state["torch_rng"])
            self.rng.bit_generator.state = state["numpy_rng"]
            self.save_dir = Path(state["save_dir"])     # model_best_* and resume.pth of one run stay in one directory
        self.global_step = int(state.get("global_step", 0))
        was = (int(state.get("freeze_stages", 0)), bool(state.get("freeze_bn", False)))
        if was != tuple(self.freeze) and self.rank == 0:       # the freeze belongs to the command line: a run may thaw stages when it resumes
            print("resume: the checkpoint was written with --freeze_stages %d%s, this run continues with --freeze_stages %d%s (the command "
                  "line wins)" % (was[0], " --freeze_bn" if was[1] else "", self.freeze[0], " --freeze_bn" if self.freeze[1] else ""), flush=True)

    def scalar_writer(self):
        """The run's scalar log (rank 0), created on first use: TensorBoard when importable, always `<dir>/scalars.jsonl` (utils/scalars.py)."""
        if self._writer is None:
            from ..utils.scalars import ScalarWriter
            self._writer = ScalarWriter(getattr(self.args, "log_dir", None) or self.save_dir) if self.rank == 0 else ScalarWriter(None)
        return self._writer

    def train(self):
        try:
            self._train()
        finally:                                                       # the TensorBoard event file and scalars.jsonl are closed with the run
            if self._writer is not None:
                self._writer.close()
                self._writer = None

    def prefill_cache(self):
        """Decode every training image and this rank's validation shard once into the device cache (each rank the whole training set: its
        training shard changes every epoch; the validation shard does not)."""
        from ..data.feeder import default_decode_workers
        from ..data.image_cache import GB
        from ..utils.distributed import shard_range
        a = self.args
        workers = getattr(a, "decode_workers", 0) or default_decode_workers(self.step.world)
        if self.dataset is not None:
            self.cache.prefill(self.dataset, workers)
        if self.valid_set is not None:
            self.cache.prefill(self.valid_set, workers, indices=range(*shard_range(len(self.valid_set), self.rank, self.step.world)))
        st = self.cache.stats()
        if self.rank == 0:
            print(f"image cache: {st['images']} images, {st['bytes_used'] / GB:.2f} GB in {st['prefill_seconds']:.1f} s, "
                  f"{st['refused']} left on the host path (budget {a.cache_images:g} GB)", flush=True)

    def _train(self):
        per_step = self.scheduler.per_step
        # --steps bounds this call's optimizer steps; under a per-step schedule, whose length it sets, the steps of the run (a resumed
        # run then ends where the uninterrupted one does)
        steps = self.step.step_count if per_step else 0
        if self.rank == 0 and (per_step or self.step.lr_mults is not None):
            mults = self.step.lr_mults
            print(f"learning rate: {self.scheduler.describe()}" + ("" if mults is None else "; per-stage multipliers " +
                  ", ".join(f"{stage} {v:g}" for stage, v in mults.items())), flush=True)
        if self.rank == 0 and not self.step.plain_adam:
            print(f"optimizer: weight decay {self.step.weight_decay:g} (convolution weights), gradient clipping at norm "
                  f"{self.step.clip_grad_norm:g}, weight EMA {self.step.ema_decay:g} (0 = off)", flush=True)
        if self.rank == 0 and self.step.optimizer != "adam":
            s = self.step
            print("update rule: " + (f"SGD, momentum {s.momentum:g}{' (Nesterov)' if s.nesterov else ''}; --weight_decay is coupled L2" if s.optimizer == "sgd"
                                     else "LAMB, trust ratio on convolution weights; biases and BatchNorm parameters step without it"), flush=True)
        if self.rank == 0 and self.step.accum_steps > 1:
            k, b, world = self.step.accum_steps, self.args.batch_size, self.step.world
            print(f"gradient accumulation: {k} batches per optimizer step, effective batch {k * b * world} ({k} x {b} x {world} rank(s)); "
                  "--steps, warm-up and schedule count optimizer steps; BatchNorm statistics are per micro-batch -- consider --freeze_bn "
                  "or --sync_bn for small batches", flush=True)
        if self.rank == 0 and self.freeze[0]:
            from .network import FREEZE_STAGES
            print(f"frozen trunk stages: {', '.join(FREEZE_STAGES[:self.freeze[0]])} (no gradient, BatchNorm on the stored statistics)"
                  + ("; frozen BatchNorm in the trainable trunk stages" if self.freeze[1] else ""), flush=True)
        if self.rank == 0 and self.step.sync_bn:
            print(f"synchronized BatchNorm: on (statistics over the global batch of {self.step.world} rank(s) x {self.args.batch_size})", flush=True)
        if self.rank == 0 and self.augment.train_tiles:
            tx, ty = self.augment.train_tiles
            print(f"train tiles: every sample is a random window of the {tx}x{ty} tile canvas (overlap {self.augment.tile_overlap}); this run's "
                  "validation shows whole frames -- measure tiled deployment with evaluate --tiles", flush=True)
        if self.cache is not None:
            self.prefill_cache()
        for epoch in range(self.start_epoch, self.args.epochs):
            if self.args.steps and steps >= self.args.steps:           # (a resumed run whose bound was reached before it was saved: no step more)
                break
            self.epoch = epoch
            losses, norms, rates, sizes = [], [], [], []               # one entry per optimizer step
            clipping = self.step.clip_grad_norm > 0
            group, micro, rate = None, 0, None                         # the open accumulation group: its loss sum (device), its batches, its rate

            def close_group():
                # the optimizer just ran: the group's mean loss (a device value, like the norm: read with the epoch's one copy below)
                losses.append(group if micro == 1 else group / micro)
                if per_step:
                    rates.append(rate)
                if clipping:
                    norms.append(self.step.grad_norm.clone())          # the status block's norm of this step
                sizes.append(micro)

            for images, targets in self.batches():
                if per_step:
                    rate = self.scheduler.apply()                      # a function of step_count: the same value for every batch of a group; no sync
                loss = self.step(images, targets)                      # (total, hm, offset, embedding) on the device: no host sync in the loop
                group = loss.clone() if group is None else group + loss
                micro += 1
                if self.step.updated:
                    close_group()
                    group, micro = None, 0
                    steps += 1
                    if self.args.steps and steps >= self.args.steps:
                        break
            if self.step.flush():                                      # --accum_steps: the epoch's last, partial group -- an epoch ends at an update
                close_group()
                steps += 1
            n = len(losses)
            rows = torch.stack(losses).tolist() if n else []           # one host sync per epoch
            norms = torch.stack(norms).tolist() if norms else []
            skipped = int(self.step.skipped_steps) if clipping else 0
            mean = [sum(r[k] for r in rows) / max(n, 1) for k in range(4)]
            if self.rank == 0:
                # trainer.py:126-133: "Loss/Train" per optimizer step at global_step (+= batch_size per step), "Learning rate" per epoch;
                # the reference's writer forces a device sync per step -- the same scalars are written here from the epoch's one copy
                writer = self.scalar_writer()
                for k, r in enumerate(rows):
                    writer.add_scalars("Loss/Train", dict(hm_loss=r[1], offset_loss=r[2], embedding_loss=r[3]), self.global_step)
                    if clipping:
                        writer.add_scalar("Gradient norm", norms[k], self.global_step)
                    if per_step:                                       # warm-up / cosine: the rate of every step
                        writer.add_scalar("Learning rate", rates[k], self.global_step)
                    self.global_step += self.args.batch_size * sizes[k]        # images of the step: its batches (one without --accum_steps)
                if not per_step:
                    writer.add_scalar("Learning rate", self.step.lr, self.global_step)
                if clipping:
                    writer.add_scalar("Skipped steps", skipped, self.global_step)
                writer.flush()
                print(f"epoch {epoch}: total {mean[0]:.5f} hm {mean[1]:.5f} offset {mean[2]:.5f} embedding {mean[3]:.5f} "
                      f"lr {self.step.lr:g} ({n} steps" + (f", {sum(sizes)} batches)" if self.step.accum_steps > 1 else ")"), flush=True)
            if epoch % 2 == 0:                                         # trainer.py:98-99
                self.valid()
            self.scheduler.step()
            self.augment.trigger_random_resize()                       # trainer.py:135: a new input size (multiple of 32) per epoch
            if self.rank == 0:                                         # state at the END of the epoch: --resume continues with epoch + 1
                self.save_dir.mkdir(parents=True, exist_ok=True)
                self.save_resume(self.save_dir / "resume.pth")
                if self.step.ema is not None:                          # model_best_* hold the averaged weights: the raw ones go here
                    self.net.save(self.save_dir / "last_model.pth")
            if self.args.steps and steps >= self.args.steps:
                break
