"""Host half of the optimizer options (AdamW decay, global-norm clipping, weight EMA): the C ABI's argument checks, the
binding, the command-line flags and the pure-Python pieces of TrainStep.  No GPU: every call below returns before a launch."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

SD_ERR_INVALID, SD_ERR_WORKSPACE, SD_ERR_ALIGN = -1, -2, -3          # include/sdnet_hip.h
f = C.c_float


def _optim(lib, param=16, grad=16, m=16, v=16, n=16, step=1, wd=0.0, mask=0, max_norm=0.0, partials=0, npartials=0, ema=0, ema_decay=0.0,
           status=0):
    return lib.sd_optim_step(param, grad, m, v, n, step, f(1e-3), f(0.9), f(0.999), f(1e-8), f(1.0), f(wd), mask, f(max_norm), partials,
                             npartials, ema, f(ema_decay), status, 0)


def test_binding_declares_the_new_symbols_and_the_library_exports_them():
    from structuredetector_amd import _lib as L
    for name in ("sd_grad_sumsq_workspace_bytes", "sd_grad_sumsq", "sd_optim_step"):
        assert name in L.declared_symbols()
        assert hasattr(L.lib(), name)


def test_optim_step_rejects_bad_arguments_with_a_message():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    assert _optim(lib, n=10) == SD_ERR_INVALID and b"sd_optim_step" in lib.sd_last_error()             # n % 4 != 0
    assert _optim(lib, step=0) == SD_ERR_INVALID
    assert _optim(lib, param=0) == SD_ERR_INVALID
    assert _optim(lib, param=8) == SD_ERR_ALIGN and b"aligned" in lib.sd_last_error()
    assert _optim(lib, ema=24, ema_decay=0.5) == SD_ERR_ALIGN
    assert _optim(lib, wd=-0.1) == SD_ERR_INVALID and b"weight_decay" in lib.sd_last_error()
    assert _optim(lib, wd=float("nan")) == SD_ERR_INVALID
    assert _optim(lib, max_norm=-1.0) == SD_ERR_INVALID and b"max_norm" in lib.sd_last_error()
    for bad in (1.0, 1.5, -0.01, float("nan")):
        assert _optim(lib, ema=16, ema_decay=bad) == SD_ERR_INVALID and b"ema_decay" in lib.sd_last_error(), bad
    assert _optim(lib, max_norm=1.0, partials=0, npartials=4, status=16) == SD_ERR_INVALID and b"partials" in lib.sd_last_error()
    assert _optim(lib, max_norm=1.0, partials=16, npartials=0, status=16) == SD_ERR_INVALID
    assert _optim(lib, max_norm=1.0, partials=16, npartials=4, status=0) == SD_ERR_INVALID
    assert _optim(lib, max_norm=1.0, partials=20, npartials=1, status=16) == SD_ERR_ALIGN
    # the count must be the one sd_grad_sumsq writes for this n (16 floats: one block, one partial)
    assert _optim(lib, max_norm=1.0, partials=16, npartials=4, status=16) == SD_ERR_INVALID and b"partials" in lib.sd_last_error()
    assert _optim(lib, n=4096, max_norm=1.0, partials=16, npartials=3, status=16) == SD_ERR_INVALID


def test_grad_sumsq_rejects_bad_arguments_and_sizes_its_workspace():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    assert lib.sd_grad_sumsq(16, 10, 16, 1 << 12, 0) == SD_ERR_INVALID and b"sd_grad_sumsq" in lib.sd_last_error()
    assert lib.sd_grad_sumsq(0, 16, 16, 1 << 12, 0) == SD_ERR_INVALID
    assert lib.sd_grad_sumsq(16, 16, 0, 1 << 12, 0) == SD_ERR_INVALID
    assert lib.sd_grad_sumsq(8, 16, 16, 1 << 12, 0) == SD_ERR_ALIGN
    assert lib.sd_grad_sumsq(16, 16, 12, 1 << 12, 0) == SD_ERR_ALIGN
    assert lib.sd_grad_sumsq(16, 1 << 20, 16, 8, 0) == SD_ERR_WORKSPACE and b"workspace" in lib.sd_last_error()
    # one double per block of 256 threads x 16 bytes, at most 512 blocks; pure host arithmetic
    assert lib.sd_grad_sumsq_workspace_bytes(0) == 0 and lib.sd_grad_sumsq_workspace_bytes(-4) == 0
    assert lib.sd_grad_sumsq_workspace_bytes(1000) == 8
    assert lib.sd_grad_sumsq_workspace_bytes(1024 + 4) == 16
    assert lib.sd_grad_sumsq_workspace_bytes(21_850_000) == 8 * 512


def test_flags_default_to_off_and_are_validated():
    from structuredetector_amd.utils.args import Arguments, finalize
    p = Arguments().parser
    ns = p.parse_args([])
    assert (ns.weight_decay, ns.clip_grad_norm, ns.ema_decay) == (0.0, 0.0, 0.0)
    ns = p.parse_args("--weight_decay 0.05 --clip_grad_norm 2.5 --ema_decay 0.999".split())
    assert (ns.weight_decay, ns.clip_grad_norm, ns.ema_decay) == (0.05, 2.5, 0.999)
    for argv, word in (("--weight_decay -0.1", "weight_decay"), ("--clip_grad_norm -1", "clip_grad_norm"), ("--ema_decay -0.5", "ema_decay"),
                       ("--ema_decay 1.0", "ema_decay")):
        with pytest.raises(AssertionError, match=word):
            finalize(p.parse_args(argv.split()))


def test_train_step_kwargs_pass_the_options_through():
    from structuredetector_amd.model.trainer import train_step_kwargs
    from structuredetector_amd.utils.args import Arguments
    p = Arguments().parser
    import inspect

    from structuredetector_amd.model.trainer import TrainStep
    sig = inspect.signature(TrainStep).parameters
    assert all(sig[k].default == 0.0 for k in ("weight_decay", "clip_grad_norm", "ema_decay"))
    assert not {"weight_decay", "clip_grad_norm", "ema_decay"} & set(train_step_kwargs(p.parse_args([])))      # off: TrainStep's own defaults
    assert set(train_step_kwargs(p.parse_args(["--ema_decay", "0.5"]))) == {"lr", "sync_bn", "ema_decay"}
    kw = train_step_kwargs(p.parse_args("--weight_decay 0.05 --clip_grad_norm 2.5 --ema_decay 0.999 -l 0.01".split()))
    assert (kw["weight_decay"], kw["clip_grad_norm"], kw["ema_decay"], kw["lr"]) == (0.05, 2.5, 0.999, 0.01)


def test_ema_warm_up_schedule():
    from structuredetector_amd.model.trainer import TrainStep
    me = SimpleNamespace(ema_decay=0.999)
    assert TrainStep.ema_decay_at(me, 1) == pytest.approx(2 / 11)
    assert TrainStep.ema_decay_at(me, 90) == pytest.approx(0.91)
    assert TrainStep.ema_decay_at(me, 100_000) == 0.999
    assert TrainStep.ema_decay_at(SimpleNamespace(ema_decay=0.1), 1) == 0.1


def test_decay_mask_flags_the_four_dimensional_tensors_only():
    """`TrainStep.build_decay_mask` on a stand-in for the flat layout (32-byte slots): one flag per group of four floats, set inside the
    slot of a 4-D tensor, clear for vectors and for the padding that follows them."""
    from structuredetector_amd.model.trainer import TrainStep
    shapes = [(8, 3, 3, 3), (8,), (8,), (5, 8, 1, 1), (5,)]
    params, off, offs = [torch.zeros(s) for s in shapes], 0, {}
    for p in params:
        offs[id(p)] = (off, p.numel())
        off += (p.numel() + 7) // 8 * 8
    net = SimpleNamespace(flat_params=torch.zeros(off), _flat_order=params, _flat_off=offs)
    mask = TrainStep.build_decay_mask(net)
    assert mask.dtype == torch.uint8 and mask.numel() == off // 4
    per_float = mask.repeat_interleave(4)
    for p in params:
        lo, n = offs[id(p)]
        assert bool(per_float[lo:lo + n].all()) == (p.dim() == 4) and bool(per_float[lo:lo + n].any()) == (p.dim() == 4)
    assert int(mask.sum()) * 4 == sum(p.numel() for p in params if p.dim() == 4)
