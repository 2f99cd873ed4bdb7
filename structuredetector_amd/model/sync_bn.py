"""Synchronized BatchNorm: the statistics exchange of `TrainStep(..., sync_bn=True)`.

Every BatchNorm of the training step finishes its batch statistics in two halves through the C ABI (include/sdnet_hip.h,
"synchronized BatchNorm"): phase 1 reduces the layer's partial rows to ONE fp64 vector per layer and direction,

    [S0 (C), S1 (C), n]      forward: S0 = sum x, S1 = sum x^2;   backward: S0 = sum g, S1 = sum g * xhat

this object sums that vector over the ranks of the process group, and phase 2 turns the global sums into the outputs (mean,
invstd and the running statistics; the two means of the backward's apply pass).  The element count travels in the vector, so
ranks with different batch sizes stay correct.  With one rank there is no collective and the split finish gives the bits of
the fused one.

The vectors live in one fp64 arena allocated once (two slots per BatchNorm layer: forward and backward, 2C + 1 doubles each);
the engine takes them in its fixed layer order, identical on every rank.  The all-reduce is issued on torch's current stream
with `async_op=True` and joined with `wait()`: with the nccl backend the compute stream waits for the collective on the device,
the host does not synchronise.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .. import _lib as L


class BnStatsExchange:
    def __init__(self, channels, device, process_group=None, world=None):
        """channels: C of every BatchNorm layer the training step finishes (any order: only the total size matters)."""
        self.channels = [int(c) for c in channels]
        self.pg = process_group
        if world is None:
            world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.world = int(world)
        self.half = sum(2 * c + 1 for c in self.channels)             # forward slots, then as many backward slots
        self.arena = torch.zeros(2 * self.half, dtype=torch.float64, device=device)
        self._off, self._end = 0, self.half
        self.log = None          # list -> one entry per phase-1 call of the step, in order (the entry point the engine used; tests)

    @classmethod
    def for_network(cls, net, process_group=None, world=None):
        from .network import BNParams
        channels = [m.c for m in net.modules() if isinstance(m, BNParams)]
        return cls(channels, net.flat_params.device, process_group, world)

    def begin(self, direction):
        """Start the forward ("fwd") or the backward ("bwd") half of the arena."""
        if direction not in ("fwd", "bwd"):
            raise ValueError(f"direction must be 'fwd' or 'bwd', got {direction!r}")
        self._off, self._end = (0, self.half) if direction == "fwd" else (self.half, 2 * self.half)

    def take(self, C):
        """The next layer's [S0 (C), S1 (C), n] slot (a view of the arena)."""
        n = 2 * int(C) + 1
        if self._off + n > self._end:
            raise L.SdError(f"BnStatsExchange: arena exhausted (a BatchNorm of {C} channels beyond the {len(self.channels)} layers it was sized for)")
        view = self.arena[self._off:self._off + n]
        self._off += n
        return view

    def record(self, name):
        if self.log is not None:
            self.log.append(name)

    def reduce(self, sums):
        """Sum `sums` over the ranks (in place); every rank ends with the same bits.  No-op with one rank."""
        if self.world > 1:
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.pg, async_op=True).wait()


def pack_sums(s0, s1, n, dtype=torch.float64):
    """[S0 (C), S1 (C), n] as one fp64 vector: the layout phase 1 writes (host-side helper for tests and tools)."""
    s0 = torch.as_tensor(s0, dtype=dtype).flatten()
    s1 = torch.as_tensor(s1, dtype=dtype).flatten()
    if s0.numel() != s1.numel():
        raise ValueError("S0 and S1 must have one value per channel each")
    return torch.cat([s0, s1, torch.tensor([float(n)], dtype=dtype)])


def unpack_sums(v):
    """(S0, S1, n) of a [S0 (C), S1 (C), n] vector."""
    C = (v.numel() - 1) // 2
    if v.numel() != 2 * C + 1:
        raise ValueError(f"not a [S0, S1, n] vector: {v.numel()} values")
    return v[:C], v[C:2 * C], float(v[2 * C])
