"""Host half of the optimizer choice (`train --optimizer {adam,sgd,lamb}`): the flags, `train_step_kwargs`, the C ABI's argument checks of
`sd_sgd_step`, `sd_lamb_step` and `sd_lamb_table_build`, the kernel-name query, the slot-table layout and `Network.optim_slots()`.  No
GPU: every entry-point call below returns before a launch.  Expected block counts and layouts are written out here by hand."""
import ctypes as C
import inspect
import re
from pathlib import Path
from types import SimpleNamespace

import pytest

ROOT = Path(__file__).resolve().parent.parent
SD_ERR_INVALID, SD_ERR_WORKSPACE, SD_ERR_ALIGN = -1, -2, -3          # include/sdnet_hip.h
OP_ADAM, OP_SGD, OP_LAMB, F_CLIP, F_EMA = 21, 30, 31, 1 << 11, 1 << 12
BLOCK, MAX_SLOT_BLOCKS = 4096, 128                                   # SD_LAMB_BLOCK_FLOATS, SD_LAMB_MAX_SLOT_BLOCKS
NAMES = ("sd_sgd_step", "sd_lamb_step", "sd_lamb_table_build", "sd_lamb_workspace_bytes")
f = C.c_float
NAN = float("nan")


def floats(*values):
    return (C.c_float * len(values))(*values)


# ---- flags ----------------------------------------------------------------------------------------------------------------------------
def test_flag_defaults_ranges_and_refusals():
    from structuredetector_amd.utils.args import AUG_FLAGS, Arguments, OptimizerOptions, check_optimizer
    p = Arguments().parser
    ns = p.parse_args([])
    assert (ns.optimizer, ns.momentum, ns.nesterov) == ("adam", 0.9, False)
    assert check_optimizer(ns) == OptimizerOptions("adam", 0.9, False)
    assert check_optimizer(SimpleNamespace()) == OptimizerOptions("adam", 0.9, False)                 # a namespace from before the flags
    assert check_optimizer(SimpleNamespace(optimizer=None, momentum=None)) == OptimizerOptions("adam", 0.9, False)
    assert not {"optimizer", "momentum", "nesterov"} & set(AUG_FLAGS)
    with pytest.raises(SystemExit):
        p.parse_args(["--optimizer", "rmsprop"])
    assert check_optimizer(p.parse_args("--optimizer sgd --momentum 0.8 --nesterov".split())) == OptimizerOptions("sgd", 0.8, True)
    assert check_optimizer(p.parse_args("--optimizer lamb".split())) == OptimizerOptions("lamb", 0.9, False)
    assert check_optimizer(p.parse_args("--optimizer sgd --momentum 0".split())) == OptimizerOptions("sgd", 0.0, False)
    for value in (0.0, 0.5, 0.999999):
        assert check_optimizer(SimpleNamespace(optimizer="sgd", momentum=value)).momentum == value
    for value in (-0.1, 1.0, 1.5, NAN, float("inf"), True, "0.9"):
        with pytest.raises(ValueError, match="momentum"):
            check_optimizer(SimpleNamespace(optimizer="sgd", momentum=value))
    with pytest.raises(ValueError, match="optimizer"):
        check_optimizer(SimpleNamespace(optimizer="adamw"))
    with pytest.raises(ValueError, match="nesterov"):
        check_optimizer(SimpleNamespace(optimizer="sgd", momentum=0.0, nesterov=True))
    text = " ".join(p.format_help().split())
    assert "--optimizer {adam,sgd,lamb}" in text and "The default is Adam's" in text and "coupled L2" in text


def test_train_step_kwargs_key_sets_and_step_signature():
    from structuredetector_amd.model.trainer import TrainStep, train_step_kwargs
    from structuredetector_amd.utils.args import Arguments
    p = Arguments().parser
    sig = inspect.signature(TrainStep).parameters
    assert (sig["optimizer"].default, sig["momentum"].default, sig["nesterov"].default) == ("adam", 0.9, False)
    assert set(train_step_kwargs(p.parse_args([]))) == {"lr", "sync_bn"}
    assert set(train_step_kwargs(p.parse_args("--optimizer adam --momentum 0.5 --nesterov".split()))) == {"lr", "sync_bn"}
    kw = train_step_kwargs(p.parse_args("--optimizer sgd --momentum 0.8 --nesterov".split()))
    assert set(kw) == {"lr", "sync_bn", "optimizer", "momentum", "nesterov"}
    assert (kw["optimizer"], kw["momentum"], kw["nesterov"]) == ("sgd", 0.8, True)
    kw = train_step_kwargs(p.parse_args("--optimizer lamb --weight_decay 0.01 --accum_steps 4".split()))
    assert set(kw) == {"lr", "sync_bn", "optimizer", "momentum", "nesterov", "weight_decay", "accum_steps"} and kw["optimizer"] == "lamb"
    with pytest.raises(ValueError, match="momentum"):
        train_step_kwargs(p.parse_args(["--optimizer", "sgd", "--momentum", "nan"]))


def test_inference_entry_points_never_read_the_flags():
    pkg = ROOT / "structuredetector_amd"
    for rel in ("cli/evaluate.py", "cli/detect.py", "model/predictor.py", "model/evaluator.py"):
        text = (pkg / rel).read_text()
        assert not re.search(r"check_optimizer|\.optimizer\b|\.momentum\b|\.nesterov\b", text), rel


# ---- header, binding, exports -----------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports():
    from structuredetector_amd import _lib as L
    header = " ".join((ROOT / "include" / "sdnet_hip.h").read_text().split())
    for text in ("#define SD_LAMB_BLOCK_FLOATS 4096", "#define SD_LAMB_MAX_SLOT_BLOCKS 128", "SD_NN_SGD = 30, SD_NN_LAMB = 31", "COUPLED L2",
                 "apex FusedLAMB ties the exclusion to weight_decay == 0", "You et al. 2020", "torch.optim.SGD with dampening 0"):
        assert text in header, text
    lib = L.lib()
    for name in NAMES:
        assert name in L.declared_symbols() and hasattr(lib, name)
        assert not re.match(r"sd_(optim_step|adam_step|bn_|cast_|col_sum)", name)
    assert len(L._SIGNATURES["sd_sgd_step"][1]) == 20 and len(L._SIGNATURES["sd_lamb_step"][1]) == 28
    assert len(L._SIGNATURES["sd_lamb_table_build"][1]) == 9
    assert lib.sd_lamb_workspace_bytes(0) == 0 and lib.sd_lamb_workspace_bytes(7) == 7 * 16


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _sgd(lib, param=16, grad=16, buf=16, n=16, momentum=0.9, nesterov=0, wd=0.0, ids=16, lr_mul=(1.0,), wd_mul=(1.0,), ngroups=None,
         max_norm=0.0, partials=0, npartials=0, ema=0, ema_decay=0.0, status=0, **_):
    lr_tab = None if lr_mul is None else floats(*lr_mul)
    wd_tab = None if wd_mul is None else floats(*wd_mul)
    ngroups = len(lr_mul) if ngroups is None else ngroups
    return lib.sd_sgd_step(param, grad, buf, n, f(1e-2), f(momentum), nesterov, f(1.0), f(wd), ids, lr_tab, wd_tab, ngroups, f(max_norm), partials,
                           npartials, ema, f(ema_decay), status, 0)


def _lamb(lib, param=16, grad=16, m=16, v=16, n=16, step=1, wd=0.0, ids=16, lr_mul=(1.0,), wd_mul=(1.0,), ngroups=None, max_norm=0.0, partials=0,
          npartials=0, ema=0, ema_decay=0.0, status=0, table=16, nslots=1, nblocks=1, ws=16, ws_bytes=16, **_):
    lr_tab = None if lr_mul is None else floats(*lr_mul)
    wd_tab = None if wd_mul is None else floats(*wd_mul)
    ngroups = len(lr_mul) if ngroups is None else ngroups
    return lib.sd_lamb_step(param, grad, m, v, n, step, f(1e-3), f(0.9), f(0.999), f(1e-8), f(1.0), f(wd), ids, lr_tab, wd_tab, ngroups, f(max_norm),
                            partials, npartials, ema, f(ema_decay), status, table, nslots, nblocks, ws, ws_bytes, 0)


@pytest.mark.parametrize("name, call", [("sd_sgd_step", _sgd), ("sd_lamb_step", _lamb)])
def test_both_entry_points_refuse_what_the_groups_form_refuses(name, call):
    """Made-up device addresses (never read: every case returns before the launch), real host tables; the refusals and codes of
    sd_optim_groups_step (tests/test_optim_groups_cpu.py), one by one."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    sixteen, seventeen = (1.0,) * 16, (1.0,) * 17

    def refused(code, word, **kw):
        assert call(lib, **kw) == code, kw
        assert name.encode() in lib.sd_last_error() and word in lib.sd_last_error(), (kw, lib.sd_last_error())

    refused(SD_ERR_INVALID, b"n % 4 == 0", n=10)
    refused(SD_ERR_INVALID, b"bad arguments", n=0)
    refused(SD_ERR_INVALID, b"bad arguments", param=0)
    refused(SD_ERR_INVALID, b"bad arguments", grad=0)
    refused(SD_ERR_ALIGN, b"aligned", param=8)
    refused(SD_ERR_ALIGN, b"aligned", grad=24)
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
    refused(SD_ERR_ALIGN, b"aligned", param=8, lr_mul=(1.0, -1.0), wd_mul=(1.0, NAN), ngroups=1)   # entries past ngroups are not read


def test_sgd_refuses_its_own_arguments():
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def refused(code, word, **kw):
        assert _sgd(lib, **kw) == code, kw
        assert b"sd_sgd_step" in lib.sd_last_error() and word in lib.sd_last_error(), (kw, lib.sd_last_error())

    for bad in (-0.1, 1.0, 2.0, NAN):
        refused(SD_ERR_INVALID, b"momentum must be in [0, 1)", momentum=bad)
    refused(SD_ERR_INVALID, b"nesterov needs momentum > 0", momentum=0.0, nesterov=1)
    refused(SD_ERR_INVALID, b"nesterov must be 0 or 1", nesterov=2)
    refused(SD_ERR_INVALID, b"momentum buffer", buf=0)
    refused(SD_ERR_ALIGN, b"aligned", buf=8)
    # momentum == 0: a null buffer is fine -- the call gets past every check of the buffer to the next refusal
    refused(SD_ERR_ALIGN, b"aligned", momentum=0.0, buf=0, param=8)


def test_lamb_refuses_its_own_arguments():
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def refused(code, word, **kw):
        assert _lamb(lib, **kw) == code, kw
        assert b"sd_lamb_step" in lib.sd_last_error() and word in lib.sd_last_error(), (kw, lib.sd_last_error())

    refused(SD_ERR_INVALID, b"step >= 1", step=0)
    refused(SD_ERR_INVALID, b"exp_avg", m=0)
    refused(SD_ERR_INVALID, b"exp_avg", v=0)
    refused(SD_ERR_ALIGN, b"aligned", m=8)
    refused(SD_ERR_ALIGN, b"aligned", v=4)
    refused(SD_ERR_INVALID, b"slot table", table=0)
    refused(SD_ERR_INVALID, b"workspace", ws=0)
    refused(SD_ERR_INVALID, b"nslots", nslots=0)
    refused(SD_ERR_INVALID, b"nslots", nslots=65537, nblocks=65537)
    refused(SD_ERR_INVALID, b"nblocks", nslots=2, nblocks=1, ws_bytes=1 << 20)
    refused(SD_ERR_INVALID, b"nblocks", nslots=1, nblocks=129, ws_bytes=1 << 20)
    refused(SD_ERR_ALIGN, b"16-byte aligned", table=8)
    refused(SD_ERR_ALIGN, b"8-byte aligned", ws=20)
    refused(SD_ERR_WORKSPACE, b"workspace too small", nslots=1, nblocks=3, ws_bytes=47)
    refused(SD_ERR_INVALID, b"2^33", n=1 << 33, table=16)


def _build(lib, lo, hi, adapt, n, nslots=None, query=False, short=0):
    """sd_lamb_table_build on host arrays -> (code, bytes needed, blocks, the table as a list of ints or None)."""
    count = len(lo) if nslots is None else nslots
    i64 = C.c_int64 * max(len(lo), 1)
    lo_a, hi_a, ad_a = i64(*lo), i64(*hi), (C.c_ubyte * max(len(adapt), 1))(*adapt)
    need, blocks = C.c_size_t(0), C.c_int(0)
    code = lib.sd_lamb_table_build(lo_a, hi_a, ad_a, count, n, None, 0, C.byref(need), C.byref(blocks))
    if code or query:
        return code, need.value, blocks.value, None
    table = (C.c_int32 * (need.value // 4))()
    code = lib.sd_lamb_table_build(lo_a, hi_a, ad_a, count, n, table, need.value - short, None, None)
    return code, need.value, blocks.value, list(table)


def test_table_helper_refusals():
    from structuredetector_amd import _lib as L
    lib = L.lib()

    def refused(code, word, *a, **kw):
        assert _build(lib, *a, **kw)[0] == code, (a, kw)
        assert b"sd_lamb_table_build" in lib.sd_last_error() and word in lib.sd_last_error(), (a, kw, lib.sd_last_error())

    need, blocks = C.c_size_t(), C.c_int()
    assert lib.sd_lamb_table_build(None, None, None, 1, 8, None, 0, C.byref(need), C.byref(blocks)) == SD_ERR_INVALID
    assert b"host arrays" in lib.sd_last_error()
    refused(SD_ERR_INVALID, b"nslots", [0], [8], [1], 8, nslots=0)
    refused(SD_ERR_INVALID, b"nslots", [0], [8], [1], 8, nslots=65537)
    refused(SD_ERR_INVALID, b"multiple of 8", [0], [12], [1], 12)
    refused(SD_ERR_INVALID, b"multiple of 8", [0], [8], [1], 0)
    refused(SD_ERR_INVALID, b"slot 0", [8], [16], [1], 16)                  # does not start at 0
    refused(SD_ERR_INVALID, b"slot 1", [0, 16], [8, 24], [1, 1], 24)        # a gap
    refused(SD_ERR_INVALID, b"slot 1", [0, 0], [8, 16], [1, 1], 16)         # an overlap
    refused(SD_ERR_INVALID, b"slot 1", [0, 8], [8, 8], [1, 1], 8)           # an empty slot
    refused(SD_ERR_INVALID, b"slot 1", [0, 8], [8, 20], [1, 1], 24)         # not whole float4 pairs
    refused(SD_ERR_INVALID, b"slot 1", [0, 8], [8, 32], [1, 1], 24)         # past the end
    refused(SD_ERR_INVALID, b"slots end at 16", [0, 8], [8, 16], [1, 1], 24)
    refused(SD_ERR_WORKSPACE, b"table needs 20 bytes", [0], [8], [1], 8, short=4)


def test_table_layout_of_a_hand_written_buffer():
    """Slots of 8, 16, one block's worth, one block + 8, three blocks + 8 and more than a sweep (129 blocks' worth: the cap of 128) floats.
    Block counts by hand: 1, 1, 1, 2, 4, 128."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    sizes = [8, 16, BLOCK, BLOCK + 8, 3 * BLOCK + 8, 129 * BLOCK]
    want_blocks = [1, 1, 1, 2, 4, 128]
    adapt = [1, 0, 1, 0, 1, 1]
    lo = [sum(sizes[:k]) for k in range(len(sizes))]
    hi = [a + s for a, s in zip(lo, sizes)]
    n = hi[-1]
    code, need, blocks, table = _build(lib, lo, hi, adapt, n)
    assert code == 0 and blocks == sum(want_blocks) == 137 and need == 4 * (4 * 6 + 137)
    assert _build(lib, lo, hi, adapt, n, query=True)[1:3] == (need, blocks)
    rows, owner = [table[4 * s:4 * s + 4] for s in range(6)], table[24:]
    first = 0
    for s, (row, nb) in enumerate(zip(rows, want_blocks)):
        assert row[0] == lo[s] // 4 and row[1] == hi[s] // 4 and row[2] == first
        assert row[3] & 0xffff == nb and (row[3] >> 30) & 1 == adapt[s] and row[3] >> 31 == 0
        assert owner[first:first + nb] == [s] * nb                          # no block spans two slots: each names exactly one
        first += nb
    assert len(owner) == 137
    # the walk of the kernels, restated: block b of a slot's nb takes lo4 + (r * nb + b) * 1024 + [0, 1024) for r = 0, 1, ...
    seen = bytearray(n // 4)
    for b, s in enumerate(owner):
        lo4, hi4, start, word = rows[s]
        nb, bi = word & 0xffff, b - start
        base = lo4 + bi * (BLOCK // 4)
        while base < hi4:
            for i in range(base, min(base + BLOCK // 4, hi4)):
                seen[i] += 1
            base += nb * (BLOCK // 4)
    assert set(seen) == {1}                                                 # every float4 of every slot exactly once
    assert lib.sd_lamb_workspace_bytes(blocks) == 137 * 16


# ---- kernel names -----------------------------------------------------------------------------------------------------------------------
def _ask(lib, op, n, flags=0, form=0, rows=0):
    from structuredetector_amd import _lib as L
    fields = dict(op=op, form=form, B=0, H=0, W=0, M=n, C=0, Co=0, relu=0, rows=rows, flags=flags, pool_fwd_pair=0)
    return lib.sd_nn_kernel_names(C.byref(L.NnCallDesc(**fields))).decode()


def test_kernel_name_query_answers_the_new_ops_and_keeps_its_unknown_ops():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    for n, grid, blocks in ((4096, 4, 4), (21_850_000, 4096, 512)):
        assert _ask(lib, OP_ADAM, n) == f"k_adam grid={grid} block=256 lds=0"                     # the SGD grid is k_adam's
        for form in (0, 1, 2):
            assert _ask(lib, OP_SGD, n, form=form) == f"k_sgd<{form}, false, false> grid={grid} block=256 lds=0"
        assert _ask(lib, OP_SGD, n, F_EMA, form=1) == f"k_sgd<1, false, true> grid={grid} block=256 lds=0"
        assert _ask(lib, OP_SGD, n, F_CLIP | F_EMA, form=2) == (f"k_grad_sumsq grid={blocks} block=256 lds=0; "
                                                                f"k_sgd<2, true, true> grid={grid} block=256 lds=0")
        assert _ask(lib, OP_LAMB, n, rows=77) == ("k_lamb_moments<false> grid=77 block=256 lds=0; k_lamb_apply<false, false> grid=77 block=256 lds=0"
                                                  " | ws_bytes=1232")
        assert _ask(lib, OP_LAMB, n, F_CLIP | F_EMA, rows=5) == (f"k_grad_sumsq grid={blocks} block=256 lds=0; k_lamb_moments<true> grid=5 block=256 lds=0; "
                                                                 "k_lamb_apply<true, true> grid=5 block=256 lds=0 | ws_bytes=80")
    for op in (OP_SGD, OP_LAMB):
        answer = _ask(lib, op, 10, rows=1)
        assert answer.startswith("refused: sd_nn_kernel_names: ") and "n % 4 == 0" in answer
    assert "form" in _ask(lib, OP_SGD, 4096, form=3) and _ask(lib, OP_SGD, 4096, form=3).startswith("refused: ")
    assert "rows" in _ask(lib, OP_LAMB, 4096) and _ask(lib, OP_LAMB, 4096).startswith("refused: ")
    for op in (24, 27, 29, 32):
        assert _ask(lib, op, 4096) == f"refused: sd_nn_kernel_names: unknown op {op}"


# ---- slots of the network -----------------------------------------------------------------------------------------------------------------
def test_optim_slots_of_a_cpu_network():
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model import Network
    from tests.test_host_cpu import make_args
    net = Network(make_args(2, 1, 20, 40), pretrained=False)
    slots = net.optim_slots()                                              # before .to(device)
    ids, groups = net.optim_groups()
    params = list(net.parameters())
    assert len(slots) == len(params)
    off = 0
    for p, (lo, hi, adapt) in zip(params, slots):
        assert lo == off and hi == off + (p.numel() + 7) // 8 * 8 and lo % 8 == 0      # `_flat_off` of `_build_flat`, rounded up to 8
        assert adapt is (p.dim() == 4)
        slot_ids = ids[lo // 4:hi // 4]
        assert bool((slot_ids == slot_ids[0]).all()) and groups[int(slot_ids[0])][1] is adapt      # one group a slot; adapted = the decayed kind
        off = hi
    assert off == ids.numel() * 4
    assert any(a for _, _, a in slots) and not all(a for _, _, a in slots)
    # the helper accepts the network's table as it is
    code, need, blocks, table = _build(L.lib(), [s[0] for s in slots], [s[1] for s in slots], [int(s[2]) for s in slots], off)
    assert code == 0 and blocks == sum(min(-(-(hi - lo) // BLOCK), MAX_SLOT_BLOCKS) for lo, hi, _ in slots)
