"""Fine-tuning with frozen trunk stages / frozen BatchNorm (`train --freeze_stages N [--freeze_bn]`, `Network.freeze`), the parts that need
no GPU: the flags and `check_freeze`, the flat-buffer range of the frozen stages, the launch plan and the refusals of the frozen-BatchNorm
backward entry point (sd_frozen_bn_bwd / sd_frozen_bn_bwd_bf16)."""
import ctypes as C
from argparse import Namespace

import pytest

INVALID = -1
OP_BN_FROZEN_BWD = 25                  # SD_NN_BN_FROZEN_BWD (include/sdnet_hip.h)


def test_parser_defaults_and_help():
    from structuredetector_amd.utils.args import Arguments
    parser = Arguments().parser
    a = parser.parse_args([])
    assert a.freeze_stages == 0 and a.freeze_bn is False
    a = parser.parse_args(["--freeze_stages", "3", "--freeze_bn"])
    assert a.freeze_stages == 3 and a.freeze_bn is True
    text = " ".join(parser.format_help().split())
    assert "--freeze_stages N" in text and "--freeze_bn" in text and "Needs --freeze_stages >= 1" in text


def test_check_freeze_answers():
    from structuredetector_amd.utils.args import check_freeze
    assert check_freeze(Namespace()) == (0, False)                                   # a namespace from before the flags
    assert check_freeze(Namespace(freeze_stages=0, freeze_bn=False)) == (0, False)
    assert check_freeze(Namespace(freeze_stages=5, freeze_bn=True)) == (5, True)
    assert check_freeze(Namespace(freeze_stages=2)) == (2, False)
    for bad in (-1, 6, 2.5, True, "2"):
        with pytest.raises(ValueError, match="freeze_stages"):
            check_freeze(Namespace(freeze_stages=bad, freeze_bn=False))
    with pytest.raises(ValueError, match="freeze_bn"):
        check_freeze(Namespace(freeze_stages=0, freeze_bn=True))
    with pytest.raises(ValueError, match="freeze_bn"):
        check_freeze(Namespace(freeze_bn=True))


def test_check_train_and_the_flag_table_do_not_know_the_flags():
    """`check_train` and AUG_FLAGS are recorded by tests/golden/augment_call_trace.json: the freeze flags have a check of their own.
    A guard (it holds without the feature too), not coverage of it."""
    from structuredetector_amd.utils import args as A
    assert not any("freeze" in name for name in A.AUG_FLAGS)
    A.check_train(Namespace(freeze_stages=99, freeze_bn=True, width=64, height=64))   # not its business


def _net():
    from structuredetector_amd.model import Network
    return Network(Namespace(labels={"a": 0, "b": 1}, parts={"p": 0}, fpn_depth=128), pretrained=False, init_weights=False)


def test_frozen_range_is_the_slot_arithmetic_of_the_flat_buffer():
    from structuredetector_amd.model.network import FREEZE_STAGES
    net = _net()
    assert FREEZE_STAGES == ("adpater", "down1", "down2", "down3", "down4")
    assert (net.frozen_stages, net.frozen_bn, net.frozen_range()) == (0, False, (0, 0))
    # the slots of _build_flat: every parameter, in the order of parameters(), at the next multiple of 8 floats
    starts, total = {}, 0
    for name, p in net.named_parameters():
        starts.setdefault(name.split(".")[0], total)
        total += (p.numel() + 7) // 8 * 8
    order = list(starts)
    assert order[:5] == list(FREEZE_STAGES) and order[5] == "up1"
    for n in range(6):
        assert net.freeze(n) is net
        assert net.frozen_stages == n and net.frozen_bn is False
        assert net.frozen_range() == (0, starts[order[n]] if n else 0), n
        frozen = {name for name, p in net.named_parameters() if not p.requires_grad}
        assert frozen == {name for name, _ in net.named_parameters() if name.split(".")[0] in FREEZE_STAGES[:n]}
    assert net.frozen_range()[1] % 8 == 0 and net.frozen_range()[1] == starts["up1"]


def test_freeze_bn_fixes_the_trunk_batchnorm_affines_only():
    net = _net().freeze(2, bn=True)
    assert (net.frozen_stages, net.frozen_bn) == (2, True)
    for name, p in net.named_parameters():
        stage = name.split(".")[0]
        trunk_bn = stage in ("down2", "down3", "down4") and (".bn" in name or ".downsample.1." in name)
        assert p.requires_grad == (stage not in ("adpater", "down1") and not trunk_bn), name
    assert all(p.requires_grad for n, p in net.named_parameters() if n.startswith(("up", "head")))
    net.freeze(0)
    assert all(p.requires_grad for p in net.parameters()) and net.frozen_range() == (0, 0)
    for bad in (-1, 6, 2.5, True):
        with pytest.raises(ValueError):
            net.freeze(bad)
    with pytest.raises(ValueError, match="stages >= 1"):
        net.freeze(0, bn=True)
    assert set(net.state_dict()) == set(_net().state_dict())                         # the keys are what they were


def _ask(**d):
    from structuredetector_amd import _lib as L
    fields = dict(op=OP_BN_FROZEN_BWD, form=0, B=0, H=0, W=0, M=0, C=0, Co=0, relu=0, rows=0, flags=15, pool_fwd_pair=0)
    fields.update(d)
    return L.lib().sd_nn_kernel_names(C.byref(L.NnCallDesc(**fields))).decode()


def test_kernel_names_answer_the_new_op():
    # all four pointers aligned: a float4 per thread, 8 bf16 per thread; the grid-stride grid is capped at 4096 blocks
    assert _ask(M=30, C=64) == "k_bn_frozen_bwd_f32x4 grid=2 block=256 lds=0"
    assert _ask(M=30, C=64, form=1) == "k_bn_frozen_bwd_bf16x8 grid=1 block=256 lds=0"
    assert _ask(M=64 * 128 * 128, C=64) == "k_bn_frozen_bwd_f32x4 grid=4096 block=256 lds=0"
    assert _ask(M=64 * 128 * 128, C=64, form=1) == "k_bn_frozen_bwd_bf16x8 grid=4096 block=256 lds=0"
    # any of dy, y, dx, g_out misaligned: the element-wise kernels
    for flags in range(15):
        assert _ask(M=30, C=64, flags=flags) == "k_bn_frozen_bwd_ew<float> grid=8 block=256 lds=0", flags
        assert _ask(M=30, C=64, form=1, flags=flags) == "k_bn_frozen_bwd_ew<unsigned short> grid=8 block=256 lds=0", flags
    assert _ask(M=30, C=4, form=1) == "k_bn_frozen_bwd_ew<unsigned short> grid=1 block=256 lds=0"          # bf16: C % 8
    assert _ask(M=30, C=4) == "k_bn_frozen_bwd_f32x4 grid=1 block=256 lds=0"
    # the family's shape checker
    assert _ask(M=30, C=6) == "refused: sd_nn_kernel_names: needs M > 0 and C in {4..1024} with C/4 dividing 256 (got M=30 C=6)"
    assert _ask(M=0, C=64).startswith("refused: sd_nn_kernel_names: needs M > 0")
    # the ids of the recorded trace have not moved: 24 is still nobody's
    assert _ask(op=24, M=30, C=64).startswith("refused: sd_nn_kernel_names: unknown op")


@pytest.mark.parametrize("name", ["sd_frozen_bn_bwd", "sd_frozen_bn_bwd_bf16"])
def test_entry_point_rejects_bad_arguments_without_touching_the_gpu(name):
    """Every refusal comes before any launch: the stand-in pointers are never read."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    assert name in L.declared_symbols()
    fn = getattr(lib, name)
    err = lambda: lib.sd_last_error().decode()
    dy, y, sc, dx, g = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    for args in ((0, y, sc, 8, 64, dx, g), (dy, y, 0, 8, 64, dx, g), (dy, y, sc, 8, 64, 0, g)):
        assert fn(*args, 0) == INVALID and err() == f"{name}: null pointer"
    assert fn(dy, y, sc, 0, 64, dx, g, 0) == INVALID and err().startswith(f"{name}: needs M > 0")
    assert fn(dy, y, sc, 8, 6, dx, g, 0) == INVALID and "(got M=8 C=6)" in err()
    alias = f"{name}: dx and g_out must not alias dy, y or each other"
    for args in ((dy, y, sc, 8, 64, dy, g), (dy, y, sc, 8, 64, y, 0), (dy, y, sc, 8, 64, dx, dy), (dy, y, sc, 8, 64, dx, y),
                 (dy, y, sc, 8, 64, dx, dx), (dy, 0, sc, 8, 64, dy + 64, 0)):                  # (the last: overlapping, not equal)
        assert fn(*args, 0) == INVALID and err() == alias, args
