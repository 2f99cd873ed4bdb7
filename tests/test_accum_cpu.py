"""Host half of gradient accumulation (`train --accum_steps K`): the flag and its check, the optimizer steps of an epoch and of a run,
the argument checks of `sd_grad_accum` and its kernel-name query.  No GPU: every entry-point call below returns before a launch.
Expected counts are written out here (ceil(n / K) by hand), never taken from the code under test."""
import ctypes as C
import inspect
from types import SimpleNamespace

import pytest

SD_ERR_INVALID, SD_ERR_ALIGN = -1, -3                                   # include/sdnet_hip.h
OP_ADAM, OP_GRAD_ACCUM = 21, 28                                         # SD_NN_ADAM, SD_NN_GRAD_ACCUM
N_FLAT = 21_850_000                                                     # the flat buffer of the flagship network, rounded


def _ask(lib, op, n, form=0):
    from structuredetector_amd import _lib as L
    fields = dict(op=op, form=form, B=0, H=0, W=0, M=n, C=0, Co=0, relu=0, rows=0, flags=0, pool_fwd_pair=0)
    return lib.sd_nn_kernel_names(C.byref(L.NnCallDesc(**fields))).decode()


# ---- flag -----------------------------------------------------------------------------------------------------------------------------
def test_flag_defaults_to_one_and_the_range_ends_are_checked():
    from structuredetector_amd.utils.args import AUG_FLAGS, MAX_ACCUM_STEPS, Arguments, check_accum
    p = Arguments().parser
    ns = p.parse_args([])
    assert ns.accum_steps == 1 and check_accum(ns) == 1 and MAX_ACCUM_STEPS == 64
    assert check_accum(SimpleNamespace()) == 1                            # a namespace from before the flag
    assert "accum_steps" not in AUG_FLAGS
    for k in (1, 2, 4, 64):
        assert check_accum(p.parse_args(["--accum_steps", str(k)])) == k
    for bad in ("0", "-1", "65"):
        with pytest.raises(ValueError, match="accum_steps"):
            check_accum(p.parse_args(["--accum_steps", bad]))
    for bad in (2.0, True, "4", float("nan")):
        with pytest.raises(ValueError, match="accum_steps"):
            check_accum(SimpleNamespace(accum_steps=bad))
    with pytest.raises(SystemExit):
        p.parse_args(["--accum_steps", "2.5"])


def test_train_step_kwargs_omit_the_key_at_one():
    from structuredetector_amd.model.trainer import TrainStep, train_step_kwargs
    from structuredetector_amd.utils.args import Arguments
    p = Arguments().parser
    assert inspect.signature(TrainStep).parameters["accum_steps"].default == 1
    assert set(train_step_kwargs(p.parse_args([]))) == {"lr", "sync_bn"}
    assert set(train_step_kwargs(p.parse_args(["--accum_steps", "1"]))) == {"lr", "sync_bn"}
    kw = train_step_kwargs(p.parse_args(["--accum_steps", "4"]))
    assert set(kw) == {"lr", "sync_bn", "accum_steps"} and kw["accum_steps"] == 4
    kw = train_step_kwargs(p.parse_args("--accum_steps 64 --weight_decay 0.05 --backbone_lr_mult 0.1 --sync_bn".split()))
    assert set(kw) == {"lr", "sync_bn", "weight_decay", "lr_mults", "accum_steps"} and kw["accum_steps"] == 64 and kw["sync_bn"] is True
    for bad in ("0", "65"):
        with pytest.raises(ValueError, match="accum_steps"):
            train_step_kwargs(p.parse_args(["--accum_steps", bad]))


def test_inference_entry_points_never_read_the_flag():
    import structuredetector_amd.cli.detect as detect
    import structuredetector_amd.cli.evaluate as evaluate
    import structuredetector_amd.model.predictor as predictor
    for module in (detect, evaluate, predictor):
        assert "accum_steps" not in inspect.getsource(module) and "check_accum" not in inspect.getsource(module), module.__name__


# ---- optimizer steps of an epoch and of a run -------------------------------------------------------------------------------------------
def test_updates_per_epoch_is_the_ceiling():
    from structuredetector_amd.utils.args import updates_per_epoch
    want = {(1, 1): 1, (7, 1): 7, (8, 1): 8, (9, 1): 9,
            (1, 4): 1, (7, 4): 2, (8, 4): 2, (9, 4): 3,
            (1, 8): 1, (7, 8): 1, (8, 8): 1, (9, 8): 2}
    for (n, k), updates in want.items():
        assert updates_per_epoch(n, k) == updates, (n, k)
    assert updates_per_epoch(0, 4) == 0 and updates_per_epoch(64, 64) == 1 and updates_per_epoch(65, 64) == 2


def test_schedule_length_and_steps_bound_count_optimizer_steps():
    from structuredetector_amd.model.trainer import LRSchedule, Trainer
    from structuredetector_amd.utils.args import run_updates
    assert run_updates(3, 9, 4) == 9 and run_updates(3, 9, 1) == 27 and run_updates(3, 9, 8) == 6
    assert run_updates(3, 9, 4, steps=5) == 5 and run_updates(3, 9, 4, steps=50) == 9 and run_updates(3, 9, 4, steps=0) == 9
    # the Trainer's three users of the count, on a stand-in that has what they read: no network, no GPU
    me = SimpleNamespace(args=SimpleNamespace(synthetic=18, batch_size=2), step=SimpleNamespace(world=1, accum_steps=4), dataset=None)
    me.batches_per_epoch = lambda: Trainer.batches_per_epoch(me)
    assert Trainer.batches_per_epoch(me) == 9 and Trainer.steps_per_epoch(me) == 3
    me.step.accum_steps = 1
    assert Trainer.steps_per_epoch(me) == 9
    me.step.world = 2                                                    # 18 images, global batch 4: four batches per rank
    assert Trainer.batches_per_epoch(me) == 4
    src = inspect.getsource(Trainer.__init__)
    assert "run_updates(args.epochs, self.batches_per_epoch(), self.step.accum_steps, args.steps)" in src
    # a cosine of that length ends exactly at the run's last optimizer step
    holder = SimpleNamespace(lr=1e-3, step_count=0)
    total = run_updates(3, 9, 4)
    sched = LRSchedule(holder, 3, schedule="cosine", warmup_steps=2, total_steps=total, min_lr=1e-5)
    assert sched.total_steps == 9 and sched.lr_at(8) > 1e-5 and sched.lr_at(9) == 1e-5
    with pytest.raises(ValueError, match="warm-up"):                     # a warm-up counted in batches (27) no longer fits the run
        LRSchedule(holder, 3, schedule="cosine", warmup_steps=9, total_steps=total)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry_point_and_the_library_exports_it():
    from structuredetector_amd import _lib as L
    assert "sd_grad_accum" in L.declared_symbols()
    assert hasattr(L.lib(), "sd_grad_accum")
    fn = L.lib().sd_grad_accum
    assert fn.restype is C.c_int and len(fn.argtypes) == 5 and fn.argtypes[2] is C.c_int64 and fn.argtypes[3] is C.c_int
    header = (__import__("pathlib").Path(__file__).resolve().parent.parent / "include" / "sdnet_hip.h").read_text()
    assert "int sd_grad_accum(float* dst, const float* src, int64_t n, int overwrite, sd_stream_t stream);" in header
    assert "SD_NN_GRAD_ACCUM = 28" in header and "SD_NN_OPTIM_GROUPS = 26" in header


def test_entry_point_rejects_bad_arguments_before_any_launch():
    """Made-up device addresses: every case returns before the launch, none is read."""
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def refused(code, word, dst=0x10000, src=0x20000, n=16, overwrite=0):
        assert lib.sd_grad_accum(dst, src, n, overwrite, 0) == code, (dst, src, n, overwrite)
        assert b"sd_grad_accum" in lib.sd_last_error() and word in lib.sd_last_error(), lib.sd_last_error()

    refused(SD_ERR_INVALID, b"n >= 0", n=-4)
    refused(SD_ERR_INVALID, b"n % 4 == 0", n=10)
    refused(SD_ERR_INVALID, b"n % 4 == 0", n=3)
    refused(SD_ERR_INVALID, b"overwrite", overwrite=2)
    refused(SD_ERR_INVALID, b"overwrite", overwrite=-1)
    refused(SD_ERR_INVALID, b"null", dst=0)
    refused(SD_ERR_INVALID, b"null", src=0)
    refused(SD_ERR_ALIGN, b"aligned", dst=0x10008)
    refused(SD_ERR_ALIGN, b"aligned", src=0x20004, overwrite=1)
    # overlapping ranges that are not the same range, from either side; touching ranges are fine (checked on the GPU)
    refused(SD_ERR_INVALID, b"overlap", dst=0x10000, src=0x10010, n=16)
    refused(SD_ERR_INVALID, b"overlap", dst=0x10010, src=0x10000, n=16, overwrite=1)
    refused(SD_ERR_INVALID, b"overlap", dst=0x10000, src=0x10000 + 4 * 4092, n=4096)
    # n == 0 succeeds without a launch and without looking at the pointers
    for dst, src, overwrite in ((0, 0, 0), (0x10000, 0x20000, 1), (0x10004, 0, 0)):
        assert lib.sd_grad_accum(dst, src, 0, overwrite, 0) == 0
    assert lib.sd_grad_accum(0, 0, 0, 2, 0) == SD_ERR_INVALID            # ... but not without looking at the mode


def test_kernel_name_query_answers_the_new_op_from_the_launchers_plan():
    """The op is 28: tests/test_optim_groups_cpu.py asks about 24 and 27 as unknown ops, so both stay nobody's."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    # a grid-stride pass over n / 4 groups of four floats, 256 threads a block: ceil(n / 4 / 256) blocks, at most 4096
    for n, grid in ((4, 1), (N_FLAT, 4096)):
        assert grid == min(-(-(n // 4) // 256), 4096)
        assert _ask(lib, OP_GRAD_ACCUM, n, form=0) == f"k_grad_accum<false> grid={grid} block=256 lds=0"
        assert _ask(lib, OP_GRAD_ACCUM, n, form=1) == f"k_grad_accum<true> grid={grid} block=256 lds=0"
        # the launch-shape helper of the optimizer kernels: the same grid as their launch over the same buffer
        assert _ask(lib, OP_ADAM, n) == f"k_adam grid={grid} block=256 lds=0"
    assert _ask(lib, OP_GRAD_ACCUM, 4 * 256 * 5 + 4) == "k_grad_accum<false> grid=6 block=256 lds=0"
    assert _ask(lib, OP_GRAD_ACCUM, 0) == ""                              # n == 0: the entry point launches nothing
    for n in (10, 3, N_FLAT + 2):
        for form in (0, 1):
            answer = _ask(lib, OP_GRAD_ACCUM, n, form)
            assert answer.startswith("refused: sd_nn_kernel_names: ") and "n % 4 == 0" in answer, answer
    assert _ask(lib, OP_GRAD_ACCUM, 16, form=2).startswith("refused: sd_nn_kernel_names: overwrite")
    for op in (24, 27, 29):                                               # 24 and 27 stay nobody's; nothing follows 28
        assert _ask(lib, op, 4096) == f"refused: sd_nn_kernel_names: unknown op {op}"
