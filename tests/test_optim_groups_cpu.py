"""Host half of the per-stage learning rates and the warm-up / cosine schedule: the C ABI's argument checks and kernel-name query of
`sd_optim_groups_step`, the command-line flags, `LRSchedule` against torch's schedulers and `Network.optim_groups()`.  No GPU: every
entry-point call below returns before a launch.  Expected schedule values come from torch.optim.lr_scheduler or from the formula written
out here, never from the code under test."""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch

SD_ERR_INVALID, SD_ERR_WORKSPACE, SD_ERR_ALIGN = -1, -2, -3          # include/sdnet_hip.h
OP_OPTIM_GROUPS, F_CLIP, F_EMA = 26, 1 << 11, 1 << 12                # SD_NN_OPTIM_GROUPS, SD_NN_CLIP, SD_NN_EMA
f = C.c_float
NAN = float("nan")


def floats(*values):
    return (C.c_float * len(values))(*values)


def _groups(lib, param=16, grad=16, m=16, v=16, n=16, step=1, wd=0.0, ids=16, lr_mul=(1.0,), wd_mul=(1.0,), ngroups=None, max_norm=0.0,
            partials=0, npartials=0, ema=0, ema_decay=0.0, status=0):
    """One call with made-up device addresses (never read: every case returns before the launch) and real host tables."""
    lr_tab = None if lr_mul is None else floats(*lr_mul)
    wd_tab = None if wd_mul is None else floats(*wd_mul)
    ngroups = len(lr_mul) if ngroups is None else ngroups
    return lib.sd_optim_groups_step(param, grad, m, v, n, step, f(1e-3), f(0.9), f(0.999), f(1e-8), f(1.0), f(wd), ids, lr_tab, wd_tab, ngroups,
                                    f(max_norm), partials, npartials, ema, f(ema_decay), status, 0)


def test_binding_declares_the_entry_point_and_the_library_exports_it():
    from structuredetector_amd import _lib as L
    assert "sd_optim_groups_step" in L.declared_symbols()
    assert hasattr(L.lib(), "sd_optim_groups_step")
    header = (__import__("pathlib").Path(__file__).resolve().parent.parent / "include" / "sdnet_hip.h").read_text()
    assert "#define SD_OPTIM_MAX_GROUPS 16" in header and "SD_NN_OPTIM_GROUPS = 26" in header


def test_groups_step_rejects_bad_arguments_with_a_message():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    sixteen, seventeen = (1.0,) * 16, (1.0,) * 17

    def refused(code, word, **kw):
        assert _groups(lib, **kw) == code, kw
        assert b"sd_optim_groups_step" in lib.sd_last_error() and word in lib.sd_last_error(), (kw, lib.sd_last_error())

    # what sd_optim_step refuses
    refused(SD_ERR_INVALID, b"n % 4 == 0", n=10)
    refused(SD_ERR_INVALID, b"step >= 1", step=0)
    refused(SD_ERR_INVALID, b"bad arguments", param=0)
    refused(SD_ERR_ALIGN, b"aligned", param=8)
    refused(SD_ERR_ALIGN, b"aligned", ema=24, ema_decay=0.5)
    refused(SD_ERR_INVALID, b"weight_decay", wd=-0.1)
    refused(SD_ERR_INVALID, b"weight_decay", wd=NAN)
    refused(SD_ERR_INVALID, b"max_norm", max_norm=-1.0)
    for bad in (1.0, 1.5, -0.01, NAN):
        refused(SD_ERR_INVALID, b"ema_decay", ema=16, ema_decay=bad)
    refused(SD_ERR_INVALID, b"partials", max_norm=1.0, partials=0, npartials=4, status=16)
    refused(SD_ERR_INVALID, b"partials", max_norm=1.0, partials=16, npartials=4, status=0)
    refused(SD_ERR_ALIGN, b"aligned", max_norm=1.0, partials=20, npartials=1, status=16)
    refused(SD_ERR_INVALID, b"partials", max_norm=1.0, partials=16, npartials=4, status=16)       # 16 floats: one block, one partial
    refused(SD_ERR_INVALID, b"partials", n=4096, max_norm=1.0, partials=16, npartials=3, status=16)
    # its own: the three tables, the group count, the multipliers
    refused(SD_ERR_INVALID, b"group_ids", ids=0)
    refused(SD_ERR_INVALID, b"lr_mul", lr_mul=None, ngroups=1)
    refused(SD_ERR_INVALID, b"wd_mul", wd_mul=None)
    refused(SD_ERR_INVALID, b"ngroups", ngroups=0)
    refused(SD_ERR_INVALID, b"ngroups", lr_mul=seventeen, wd_mul=seventeen)
    refused(SD_ERR_INVALID, b"ngroups", ngroups=-1)
    refused(SD_ERR_INVALID, b"lr_mul[1]", lr_mul=(1.0, -0.5), wd_mul=(1.0, 1.0))
    refused(SD_ERR_INVALID, b"lr_mul[0]", lr_mul=(NAN, 1.0), wd_mul=(1.0, 1.0))
    refused(SD_ERR_INVALID, b"lr_mul[15]", lr_mul=(1.0,) * 15 + (float("inf"),), wd_mul=sixteen)
    refused(SD_ERR_INVALID, b"wd_mul[1]", lr_mul=(1.0, 1.0), wd_mul=(0.0, -1.0))
    refused(SD_ERR_INVALID, b"wd_mul[0]", lr_mul=(1.0, 1.0), wd_mul=(NAN, 0.0))
    # entries past ngroups are not read as multipliers
    refused(SD_ERR_ALIGN, b"aligned", param=8, lr_mul=(1.0, -1.0), wd_mul=(1.0, NAN), ngroups=1)


def _ask(lib, op, n, flags=0):
    from structuredetector_amd import _lib as L
    fields = dict(op=op, form=0, B=0, H=0, W=0, M=n, C=0, Co=0, relu=0, rows=0, flags=flags, pool_fwd_pair=0)
    return lib.sd_nn_kernel_names(C.byref(L.NnCallDesc(**fields))).decode()


def test_kernel_name_query_answers_the_new_op_and_keeps_its_unknown_ops():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    # grid-stride pass over n / 4 groups: ceil(n / 4 / 256) blocks, at most 4096; the norm's partials: at most 512 blocks
    for n, grid, blocks in ((4096, 4, 4), (21_850_000, 4096, 512)):
        assert _ask(lib, OP_OPTIM_GROUPS, n) == f"k_optim_groups<false, false> grid={grid} block=256 lds=0"
        assert _ask(lib, OP_OPTIM_GROUPS, n, F_EMA) == f"k_optim_groups<false, true> grid={grid} block=256 lds=0"
        assert _ask(lib, OP_OPTIM_GROUPS, n, F_CLIP) == (f"k_grad_sumsq grid={blocks} block=256 lds=0; "
                                                        f"k_optim_groups<true, false> grid={grid} block=256 lds=0")
        assert _ask(lib, OP_OPTIM_GROUPS, n, F_CLIP | F_EMA) == (f"k_grad_sumsq grid={blocks} block=256 lds=0; "
                                                                f"k_optim_groups<true, true> grid={grid} block=256 lds=0")
        assert lib.sd_grad_sumsq_workspace_bytes(n) == 8 * blocks
    assert _ask(lib, OP_OPTIM_GROUPS, 10).startswith("refused: sd_nn_kernel_names: ") and "n % 4 == 0" in _ask(lib, OP_OPTIM_GROUPS, 10)
    for op in (24, 27):
        assert _ask(lib, op, 4096) == f"refused: sd_nn_kernel_names: unknown op {op}"


# ---- flags ----------------------------------------------------------------------------------------------------------------------------
def test_flags_default_to_off_and_every_range_end_is_checked():
    from structuredetector_amd.utils.args import AUG_FLAGS, Arguments, LrOptions, check_lr, stage_lr_mults
    p = Arguments().parser
    ns = p.parse_args([])
    assert (ns.lr_schedule, ns.warmup_steps, ns.min_lr, ns.backbone_lr_mult, ns.lr_layer_decay) == ("step", 0, 0.0, 1.0, 1.0)
    assert check_lr(ns) == LrOptions("step", 0, 0.0, 1.0, 1.0)
    assert check_lr(SimpleNamespace(learning_rate=1e-3)) == LrOptions("step", 0, 0.0, 1.0, 1.0)        # a namespace from before the flags
    assert not {"lr_schedule", "warmup_steps", "min_lr", "backbone_lr_mult", "lr_layer_decay"} & set(AUG_FLAGS)
    with pytest.raises(SystemExit):
        p.parse_args(["--lr_schedule", "linear"])
    ns = p.parse_args("--lr_schedule cosine --warmup_steps 100 --min_lr 1e-5 --backbone_lr_mult 0.1 --lr_layer_decay 0.8 --lr_step 5".split())
    assert check_lr(ns) == LrOptions("cosine", 100, 1e-5, 0.1, 0.8)                                   # an explicit --lr_step is accepted
    good = (("warmup_steps", 0), ("min_lr", 0.0), ("min_lr", 1e-3), ("backbone_lr_mult", 0.0), ("backbone_lr_mult", 10.0),
            ("lr_layer_decay", 1.0), ("lr_layer_decay", 1e-9))
    for name, value in good:
        ns = p.parse_args([])
        setattr(ns, name, value)
        assert getattr(check_lr(ns), name) == value
    bad = (("lr_schedule", "linear"), ("warmup_steps", -1), ("warmup_steps", 2.5), ("warmup_steps", NAN), ("warmup_steps", True),
           ("min_lr", -1e-9), ("min_lr", 1.0000001e-3), ("min_lr", NAN), ("backbone_lr_mult", -0.1), ("backbone_lr_mult", 10.5),
           ("backbone_lr_mult", NAN), ("lr_layer_decay", 0.0), ("lr_layer_decay", 1.01), ("lr_layer_decay", -0.5), ("lr_layer_decay", NAN))
    for name, value in bad:
        ns = p.parse_args([])
        setattr(ns, name, value)
        with pytest.raises(ValueError, match=name):
            check_lr(ns)
    # trunk stage s: M * D ** (5 - s); FPN and head 1; both 1: nothing is passed
    assert stage_lr_mults(1.0, 1.0) is None
    assert stage_lr_mults(0.1, 1.0) == dict(adpater=0.1, down1=0.1, down2=0.1, down3=0.1, down4=0.1, fpn=1.0, head=1.0)
    got = stage_lr_mults(0.1, 0.5)
    assert got == dict(adpater=0.1 * 0.5 ** 5, down1=0.1 * 0.5 ** 4, down2=0.1 * 0.5 ** 3, down3=0.1 * 0.5 ** 2, down4=0.1 * 0.5, fpn=1.0, head=1.0)
    assert list(got) == ["adpater", "down1", "down2", "down3", "down4", "fpn", "head"]


def test_train_step_kwargs_key_sets_off_and_on():
    import inspect

    from structuredetector_amd.model.trainer import TrainStep, train_step_kwargs
    from structuredetector_amd.utils.args import Arguments
    p = Arguments().parser
    assert inspect.signature(TrainStep).parameters["lr_mults"].default is None
    assert set(train_step_kwargs(p.parse_args([]))) == {"lr", "sync_bn"}
    # the schedule belongs to the Trainer: it never reaches the step's keyword arguments
    assert set(train_step_kwargs(p.parse_args("--lr_schedule cosine --warmup_steps 5 --min_lr 1e-5".split()))) == {"lr", "sync_bn"}
    assert set(train_step_kwargs(p.parse_args("--backbone_lr_mult 1 --lr_layer_decay 1".split()))) == {"lr", "sync_bn"}
    kw = train_step_kwargs(p.parse_args(["--backbone_lr_mult", "0.1"]))
    assert set(kw) == {"lr", "sync_bn", "lr_mults"} and kw["lr_mults"]["down4"] == 0.1 and kw["lr_mults"]["head"] == 1.0
    kw = train_step_kwargs(p.parse_args("--lr_layer_decay 0.5 --weight_decay 0.05".split()))
    assert set(kw) == {"lr", "sync_bn", "weight_decay", "lr_mults"} and kw["lr_mults"]["adpater"] == 0.5 ** 5
    with pytest.raises(ValueError, match="backbone_lr_mult"):
        train_step_kwargs(p.parse_args(["--backbone_lr_mult", "nan"]))


def test_lr_mults_of_the_step_are_checked():
    from structuredetector_amd.model.trainer import TrainStep
    assert TrainStep.check_lr_mults(None) is None
    assert TrainStep.check_lr_mults({"down1": 0.5}) == dict(adpater=1.0, down1=0.5, down2=1.0, down3=1.0, down4=1.0, fpn=1.0, head=1.0)
    for bad in ({"neck": 1.0}, {"head": -1.0}, {"head": NAN}, {"fpn": float("inf")}):
        with pytest.raises(ValueError, match="lr_mults"):
            TrainStep.check_lr_mults(bad)


# ---- schedule -------------------------------------------------------------------------------------------------------------------------
class _Step:
    def __init__(self, lr=1e-3):
        self.lr, self.step_count = lr, 0


def _torch_values(make, steps, lr=1e-3):
    """The learning rates a torch scheduler hands an optimizer for `steps` optimizer steps on a dummy CPU parameter."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = make(opt)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


def _run(schedule, steps, per_epoch=None):
    """What the training loop does: apply() before every step under a per-step schedule, step() after each `per_epoch` steps."""
    out = []
    for i in range(steps):
        if schedule.per_step:
            schedule.apply()
        out.append(schedule.step_obj.lr)
        schedule.step_obj.step_count += 1
        if per_epoch and (i + 1) % per_epoch == 0:
            schedule.step()
    return out


def test_step_schedule_without_warm_up_is_todays_steplr_bit_for_bit():
    from structuredetector_amd.model.trainer import LRSchedule
    want = _torch_values(lambda opt: torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.1), 12)     # one "optimizer step" per epoch
    obj = _Step()
    mine = LRSchedule(obj, 3)
    assert not mine.per_step
    got = []
    for epoch in range(12):
        got.append(obj.lr)
        mine.step()
    assert got == [1e-3 * 0.1 ** (e // 3) for e in range(12)]               # the expression of the class this one replaces: the same bits
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-12 * b
    assert obj.lr == 1e-3 * 0.1 ** 4


def test_warm_up_alone_is_torch_linear_lr():
    from structuredetector_amd.model.trainer import LRSchedule
    for n in (2, 5, 100):
        want = _torch_values(lambda opt: torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0 / n, total_iters=n - 1), n + 20)
        got = _run(LRSchedule(_Step(), 1000, schedule="step", warmup_steps=n, total_steps=n + 20), n + 20)
        assert got[0] == 1e-3 * (1 / n) and got[n - 1] == 1e-3 and got[-1] == 1e-3
        for a, b in zip(got, want):
            assert abs(a - b) <= 1e-12 * b, (n, a, b)


def test_warm_up_multiplies_the_step_schedule_of_the_epoch():
    from structuredetector_amd.model.trainer import LRSchedule
    got = _run(LRSchedule(_Step(), 1, schedule="step", warmup_steps=6, total_steps=12), 12, per_epoch=4)
    want = [1e-3 * 0.1 ** (i // 4) * (min(i + 1, 6) / 6 if i < 6 else 1.0) for i in range(12)]
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-12 * b


@pytest.mark.parametrize("total, min_lr", [(50, 0.0), (50, 1e-5), (7, 1e-4)])
def test_cosine_without_warm_up_is_torch_cosine_annealing(total, min_lr):
    from structuredetector_amd.model.trainer import LRSchedule
    want = _torch_values(lambda opt: torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=total, eta_min=min_lr), total)
    got = _run(LRSchedule(_Step(), 3, schedule="cosine", total_steps=total, min_lr=min_lr), total + 3, per_epoch=5)
    assert got[0] == 1e-3 and got[total:] == [min_lr] * 3                   # from T on: min_lr
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-12 * b, (a, b)


def test_cosine_with_warm_up_follows_the_formula():
    from structuredetector_amd.model.trainer import LRSchedule
    base, min_lr, n, t = 1e-3, 1e-5, 4, 15
    got = _run(LRSchedule(_Step(base), 3, schedule="cosine", warmup_steps=n, total_steps=t, min_lr=min_lr), t + 2, per_epoch=5)
    for i, a in enumerate(got):
        if i < n:
            want = base * (i + 1) / n
        elif i < t:
            want = min_lr + (base - min_lr) * 0.5 * (1 + math.cos(math.pi * (i - n) / (t - n)))
        else:
            want = min_lr
        assert abs(a - want) <= 1e-15 * base, (i, a, want)
    assert got[n - 1] == base == got[n] and got[t - 1] > min_lr and all(x > y for x, y in zip(got[n:t], got[n + 1:t + 1]))
    with pytest.raises(ValueError, match="warm-up"):
        LRSchedule(_Step(), 3, schedule="cosine", warmup_steps=15, total_steps=15)
    with pytest.raises(ValueError, match="warm-up"):
        LRSchedule(_Step(), 3, schedule="step", warmup_steps=20, total_steps=15)
    with pytest.raises(ValueError, match="schedule"):
        LRSchedule(_Step(), 3, schedule="linear")


def test_schedule_state_dict_round_trip_old_files_and_mismatch():
    from structuredetector_amd.model.trainer import LRSchedule
    kw = dict(schedule="cosine", warmup_steps=3, total_steps=20, min_lr=1e-5)
    a = LRSchedule(_Step(), 2, **kw)
    _run(a, 8, per_epoch=4)
    state = a.state_dict()
    assert set(state) == {"epoch", "base", "step_size", "gamma", "schedule", "warmup_steps", "total_steps", "min_lr"}
    obj = _Step(0.5)
    obj.step_count = 8                                                    # what the optimizer state carries
    b = LRSchedule(obj, 7, **kw)
    b.load_state_dict(state)
    assert (b.epoch, b.base, b.step_size) == (2, 1e-3, 2) and obj.lr == b.lr_at(8)
    assert _run(b, 12) == _run(a, 12)                                     # the same curve from there on
    # a file from before the options: today's four keys, loaded with the options off
    old = {"epoch": 4, "base": 1e-3, "step_size": 3, "gamma": 0.1}
    c = LRSchedule(_Step(), 9)
    c.load_state_dict(old)
    assert c.epoch == 4 and c.step_obj.lr == 1e-3 * 0.1 ** (4 // 3) and not c.per_step
    c2 = LRSchedule(_Step(), 9, total_steps=500)                          # the step schedule does not use the total: another --epochs resumes
    c2.load_state_dict(dict(state, schedule="step", warmup_steps=0, min_lr=0.0))
    with pytest.raises(ValueError, match=r"(?s)--lr_schedule step.*--lr_schedule cosine"):
        LRSchedule(_Step(), 3, **kw).load_state_dict(old)
    for change in (dict(total_steps=21), dict(warmup_steps=2), dict(min_lr=0.0), dict(schedule="step")):
        with pytest.raises(ValueError, match="resume"):
            LRSchedule(_Step(), 2, **dict(kw, **change)).load_state_dict(state)
    with pytest.raises(ValueError, match=r"(?s)over 20 optimizer steps.*over 21"):
        LRSchedule(_Step(), 2, **dict(kw, total_steps=21)).load_state_dict(state)


# ---- groups of the network ------------------------------------------------------------------------------------------------------------
def test_optim_groups_of_a_cpu_network():
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.network import FREEZE_STAGES, OPTIM_STAGES
    from structuredetector_amd.model.trainer import TrainStep
    from tests.test_host_cpu import make_args
    net = Network(make_args(2, 1, 20, 40), pretrained=False)
    ids, groups = net.optim_groups()
    assert OPTIM_STAGES == FREEZE_STAGES + ("fpn", "head")
    assert len(groups) == 14 and groups == [(stage, decayed) for stage in OPTIM_STAGES for decayed in (False, True)]
    # the flat layout (32-byte slots in registration order), restated: the stand-in `build_decay_mask` reads
    params, off, offs = list(net.parameters()), 0, {}
    for p in params:
        offs[id(p)] = (off, p.numel())
        off += (p.numel() + 7) // 8 * 8
    assert ids.dtype == torch.uint8 and ids.numel() == off // 4 and int(ids.max()) == 13
    mask = TrainStep.build_decay_mask(SimpleNamespace(flat_params=torch.zeros(off), _flat_order=params, _flat_off=offs))
    decayed = torch.tensor([d for _, d in groups], dtype=torch.uint8)
    assert torch.equal(decayed[ids.long()], mask)                         # the decay bit, element for element
    # every parameter's slot (padding included) carries one id: that of its stage and kind
    stage_of = {}
    for k, stage in enumerate(OPTIM_STAGES):
        for name in (("up1", "up2", "up3", "up4") if stage == "fpn" else (stage,)):
            for p in getattr(net, name).parameters():
                stage_of[id(p)] = k
    assert len(stage_of) == len(params)
    seen = set()
    for p in params:
        lo, n = offs[id(p)]
        slot = ids[lo // 4:(lo + (n + 7) // 8 * 8) // 4]
        assert slot.numel() and bool((slot == slot[0]).all()) and int(slot[0]) == 2 * stage_of[id(p)] + int(p.dim() == 4)
        seen.add(int(slot[0]))
    assert seen == set(range(14))                                         # every stage has weights and vectors
    stages = (ids // 2).long()
    assert bool((stages[1:] >= stages[:-1]).all())                        # stages lie one behind the other along the buffer
