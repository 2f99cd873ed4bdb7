"""The dispatch of the BatchNorm / pool / head / optimizer host layer (the tail of csrc/sd_nn.hip), asked on the CPU: no GPU, no pointer is
ever dereferenced.

* sd_nn_kernel_names prints, for every call of tests/golden/nn_call_trace.json, the launch sequence the kernel trace of the recorded commit
  holds (kernel names as rocprofv3 prints them, grids, 256 threads per block), and refuses the shapes that commit refused;
* its rpb / nb / fold / offset values equal the restatements in tests/bn_ref.py (plan, fold_plan) and tests/pool_ref.py (bwd_plan,
  fwd_kernel), which merged pull requests checked against the library on the GPU;
* every refusal keeps its code and text, and the size queries equal the plan around every threshold of red_rows and fold_rows.

The trace's LDS column is the kernel's static allocation (rocprofv3 leaves the dynamic bytes of a launch out), one constant per kernel; the
query prints the dynamic bytes, restated here per kernel (DYNAMIC_LDS)."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import pytest

from tests import bn_ref as R
from tests import pool_ref as P

ROOT = Path(__file__).resolve().parent.parent
INVALID, WORKSPACE, ALIGN = -1, -2, -3


def _tool():
    spec = importlib.util.spec_from_file_location("nn_trace", ROOT / "tools" / "nn_trace.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


TOOL = _tool()
FX = TOOL.load_fixture()
OP = {name: i for i, name in enumerate(TOOL.OPS)}
# dynamic LDS bytes of the kernels that take any, from (C, Co)
DYNAMIC_LDS = {
    "k_head_fwd": lambda c, co: (64 * (c + 4) + co * c) * 4,
    "k_head_fwd_bf16": lambda c, co: (64 * (c + 4) + co * c) * 4,
    "k_head_dgrad<float>": lambda c, co: co * c * 4,
    "k_head_dgrad<unsigned short>": lambda c, co: co * c * 4,
    "k_head_fwd_f32_c128": lambda c, co: 4 * 4 * 2048 * 4,                # four waves x four stages x 8 KB
    "k_head_wgrad_f32_c128": lambda c, co: 4 * 4 * (2048 + 256) * 4,      # ... x 9 KB
}
# what the query prints for the kernels of sd_head_wide.hip (their grids need the device)
WIDE = {"k_headw_fwd_f32": "head_wide_fwd", "k_headw_fwd_bf16": "head_wide_fwd_bf16", "k_headw_wgrad": "head_wide_wgrad", "k_headw_dgrad": "head_wide_dgrad"}


@pytest.fixture(scope="module")
def lib():
    from structuredetector_amd import _lib as L
    return L.lib()


def ask(lib, desc):
    from structuredetector_amd import _lib as L
    d = desc if isinstance(desc, dict) else dict(zip(TOOL.DESC_FIELDS, desc))
    return lib.sd_nn_kernel_names(C.byref(L.NnCallDesc(**d))).decode()


def parse(text):
    """'<launch>; <launch> | k=v k=v' -> ([(kernel, grid, lds) or (placeholder, None, None)], {k: int})."""
    head, _, tail = text.partition(" | ")
    launches = []
    for item in head.split("; "):
        m = re.fullmatch(r"(.*) grid=(\d+) block=256 lds=(\d+)", item)
        launches.append((m.group(1), int(m.group(2)), int(m.group(3))) if m else (item, None, None))
    return launches, {k: int(v) for k, v in (kv.split("=") for kv in tail.split())}


def field(call, name):
    return call["desc"][TOOL.DESC_FIELDS.index(name)]


def test_the_fixture_holds_every_entry_point_of_the_layer():
    from structuredetector_amd import _lib as L
    driven = {"sd_" + c["name"].split("/")[0] for c in FX["calls"]}
    layer = {s for s in L.declared_symbols() if re.match(r"sd_(bn_|col_sum|maxpool|upsample2x|cast_|head_(fwd|bwd)|adam_step|grad_sumsq$|optim_step)", s)}
    assert layer - driven - {"sd_bn_finalize_scratch_rows", "sd_head_bwd_workspace_bytes"} == set()
    assert {field(c, "op") for c in FX["calls"]} == set(range(len(TOOL.OPS)))


def test_query_prints_the_recorded_launch_sequence_of_every_call(lib):
    static = {}
    for call in FX["calls"]:
        text = ask(lib, call["desc"])
        if call["rc"]:
            assert call["rc"] == INVALID and not call["launches"] and text.startswith("refused: sd_nn_kernel_names: "), (call["name"], text)
            # the same reason, under the query's own name (the flat ops state "n % 4 == 0" in a text of their own)
            reason, want = text.split(": ", 2)[2], call["error"].split(": ", 1)[1]
            assert reason == want or ("n % 4 == 0" in reason and "n % 4 == 0" in want), (call["name"], text, call["error"])
            continue
        got, _ = parse(text)
        want = [re.fullmatch(r"(.*) grid=(\d+) block=256 lds=(\d+)", item).groups() for item in TOOL.fixture_launches(FX, call)]
        assert len(got) == len(want), (call["name"], text, want)
        for (kernel, grid, lds), (wkernel, wgrid, wlds) in zip(got, want):
            if grid is None:                                                # a wide head's own kernel
                assert WIDE[wkernel.split("<")[0]] == kernel, (call["name"], text, want)
                continue
            assert (kernel, grid) == (wkernel, int(wgrid)), (call["name"], text, want)
            assert lds == (DYNAMIC_LDS[kernel](field(call, "C"), field(call, "Co")) if kernel in DYNAMIC_LDS else 0), (call["name"], text)
            assert static.setdefault(kernel, wlds) == wlds                  # the trace's column: one constant per kernel


def test_query_plans_equal_the_restated_ones(lib):
    checked = set()
    for call in FX["calls"]:
        if call["rc"]:
            continue
        op, form, flags, C_ = field(call, "op"), field(call, "form"), field(call, "flags"), field(call, "C")
        launches, plan = parse(ask(lib, call["desc"]))
        kernels = [k for k, _, _ in launches]
        if op in (OP["bn_train_stats"], OP["col_sum"], OP["bn_bwd"], OP["bn_bwd_reduce"]):
            M = field(call, "M")
            wide = "k_col_reduce_bwd_bf16x8" in kernels
            want = R.plan(M, C_, elems=8 if wide else 4)
            assert (plan["rpb"], plan["nb"], plan["ws_bytes"]) == (want.rpb, want.nb, want.workspace_bytes), call["name"]
            fold = want.fold
        elif op in (OP["stem_bwd"], OP["stem_bwd_reduce"]):
            B, H, W = field(call, "B"), field(call, "H"), field(call, "W")
            want = P.bwd_plan(B, H, W, C_)
            assert (plan["rpb"], plan["nb"]) == (P.RED_ROWS_PER_BLOCK, want.nb) and plan["ws_bytes"] == R.plan(want.M, C_).workspace_bytes, call["name"]
            assert ("quad" in kernels[0]) == want.quad, call["name"]
            fold = want.fold
        elif op in (OP["bn_finalize_stats"], OP["bn_bwd_finalize"]):
            fold = R.fold_plan(field(call, "rows"), C_, scratch=bool(flags & TOOL.F_SCRATCH))
            assert (plan["slab"], plan["rows"]) == ((fold.slab, fold.rows_out) if fold else (0, field(call, "rows"))), call["name"]
            assert ("k_rows_fold" in kernels) == (fold is not None)
            checked.add(op)
            continue
        elif op == OP["bn_relu_maxpool_fwd"]:
            want = P.fwd_kernel(field(call, "W"), C_, bool(form), pair_option=bool(field(call, "pool_fwd_pair")))
            assert ("_pair<" in kernels[0]) == (want == "pair"), call["name"]
            checked.add(op)
            continue
        else:
            continue
        checked.add(op)
        assert (plan["slab"], plan["rows"]) == ((fold.slab, fold.rows_out) if fold else (0, plan["nb"])), call["name"]
        assert ("k_rows_fold" in kernels) == (fold is not None), call["name"]
        assert (plan["partial_at"], plan["means_at"], plan["fold_at"]) == (0, plan["nb"] * 2 * C_, (plan["nb"] + 1) * 2 * C_), call["name"]
        assert (plan["fold_at"] + (plan["rows"] if fold else 0) * 2 * C_) * 4 <= plan["ws_bytes"], call["name"]
    assert len(checked) == 9


def test_alignment_predicates(lib):
    """One predicate per kernel choice: every pointer it names must be 16-byte aligned, and no other."""
    def first(**d):
        return parse(ask(lib, dict(dict.fromkeys(TOOL.DESC_FIELDS, 0), **d)))[0][0][0]
    bn = dict(form=1, M=64, C=64)
    for flags in range(16):
        assert (first(op=OP["bn_bwd"], flags=flags, **bn) == "k_col_reduce_bwd_bf16x8") == (flags == 15)
        assert (first(op=OP["bn_bwd_apply"], flags=flags, **bn) == "k_bn_bwd_apply_bf16x8") == (flags == 15)
        assert (first(op=OP["bn_bwd_reduce"], flags=flags, **bn) == "k_col_reduce_bwd_bf16x8") == (flags & 3 == 3)       # dy / x alone
        assert (first(op=OP["bn_apply"], flags=flags, **bn) == "k_bn_apply_bf16x8") == (flags & 7 == 7)
        assert ("_pair<" in first(op=OP["bn_relu_maxpool_fwd"], flags=flags, B=1, H=8, W=8, C=8, pool_fwd_pair=1)) == (flags & 7 == 7)
        assert (first(op=OP["head_fwd"], flags=flags, B=1, H=64, C=128, Co=8) == "k_head_fwd_f32_c128") == (flags & 7 == 7)
        assert (first(op=OP["head_fwd"], form=1, flags=flags, B=1, H=64, C=128, Co=8) == "k_head_fwd_bf16_c128<false>") == (flags & 5 == 5)
        assert (first(op=OP["head_bwd"], flags=flags, B=1, H=64, C=128, Co=8) == "k_head_wgrad_f32_c128") == (flags & 3 == 3)
    assert first(op=OP["bn_bwd"], flags=15, relu=1, **bn) == "k_col_reduce<1, unsigned short>"          # relu = 1 reads y as bf16
    assert first(op=OP["bn_bwd"], flags=15, form=1, M=64, C=4) == "k_col_reduce<1, unsigned short>"    # C % 8
    assert first(op=OP["head_fwd"], flags=15, B=1, H=64, C=128, Co=17) == "k_head_fwd"
    assert first(op=OP["head_fwd"], form=1, flags=15, B=1, H=64, C=128, Co=17) == "k_head_fwd_bf16_c128<true>"
    assert first(op=OP["head_bwd"], flags=15, B=1, H=72, C=128, Co=8) == "k_head_wgrad"                 # HW % 16
    assert ask(lib, dict(dict.fromkeys(TOOL.DESC_FIELDS, 0), op=len(TOOL.OPS))).startswith("refused: sd_nn_kernel_names: unknown op")


def test_refusals_keep_their_code_and_text(lib):
    f = C.c_float
    p, ws = 0x1000, 1 << 30                               # a stand-in pointer (every refusal comes before any launch) and a large workspace
    err = lambda: lib.sd_last_error().decode()
    # bad C
    assert lib.sd_bn_train_stats(p, 100, 6, f(1e-5), f(0.1), p, p, p, p, p, ws, 0) == INVALID
    assert err() == "sd_bn_train_stats: needs M > 0 and C in {4..1024} with C/4 dividing 256 (got M=100 C=6)"
    assert lib.sd_col_sum_bf16(p, 100, 2048, p, 0, p, ws, 0) == INVALID
    assert err() == "sd_col_sum_bf16: needs M > 0 and C in {4..1024} with C/4 dividing 256 (got M=100 C=2048)"
    assert lib.sd_bn_stats_from_sums(p, 12, f(1e-5), f(0.1), p, p, p, p, 0) == INVALID and "(got M=1 C=12)" in err()
    assert lib.sd_maxpool_bn_relu_bwd_apply(p, p, p, 1, 4, 4, 6, p, p, p, p, p, p, 0) == INVALID and err().startswith("sd_maxpool_bn_relu_bwd_apply: needs M > 0")
    # relu out of range, and the pointers a relu form needs
    bwd = lambda name, relu, y, beta=p: getattr(lib, name)(p, p, y, relu, 64, 64, p, p, p, beta, p, p, p, p, 0, p, ws, 0)
    for name in ("sd_bn_bwd", "sd_bn_bwd_bf16"):
        assert bwd(name, 4, p) == INVALID
        assert err() == f"{name}: relu must be 0 (none), 1 (mask from y), 2 (mask recomputed from x) or 3 (mask bytes)"
        for relu, y, beta in ((1, 0, p), (3, 0, p), (2, p, 0)):
            assert bwd(name, relu, y, beta) == INVALID and err() == f"{name}: null pointer"
    assert lib.sd_bn_bwd_apply_bf16(p, p, p, -1, 64, 64, p, p, p, p, p, p, p, 0) == INVALID and err().startswith("sd_bn_bwd_apply_bf16: relu must be")
    assert lib.sd_bn_bwd_reduce(p, p, p, 7, 64, 64, p, p, p, p, p, p, 0, p, p, ws, 0) == INVALID and err().startswith("sd_bn_bwd_reduce: relu must be")
    # misaligned sums
    text = ": the fp64 sums must be 8-byte aligned"
    assert lib.sd_bn_train_sums(p, 64, 64, p + 4, p, ws, 0) == ALIGN and err() == "sd_bn_train_sums" + text
    assert lib.sd_bn_stats_sums(p, 8, 64, 64, p + 4, 0, 0) == ALIGN and err() == "sd_bn_stats_sums" + text
    assert lib.sd_bn_bwd_sums(p, 8, 64, 64, p, p, 0, p + 4, 0, 0) == ALIGN and err() == "sd_bn_bwd_sums" + text
    assert lib.sd_bn_bwd_reduce_bf16(p, p, p, 0, 64, 64, p, p, p, p, p, p, 0, p + 4, p, ws, 0) == ALIGN and err() == "sd_bn_bwd_reduce_bf16" + text
    assert lib.sd_maxpool_bn_relu_bwd_reduce(p, p, p, 1, 4, 4, 64, p, p, p, p, p, p, 0, p + 4, p, ws, 0) == ALIGN and err() == "sd_maxpool_bn_relu_bwd_reduce" + text
    assert lib.sd_bn_stats_from_sums(p + 4, 64, f(1e-5), f(0.1), p, p, p, p, 0) == ALIGN and err() == "sd_bn_stats_from_sums" + text
    assert lib.sd_bn_bwd_means_from_sums(p + 4, 64, p, 0) == ALIGN and err() == "sd_bn_bwd_means_from_sums" + text
    # short workspace: one byte less than the size query's answer
    need = lib.sd_col_reduce_workspace_bytes(4096, 64)
    assert lib.sd_bn_train_stats_bf16(p, 4096, 64, f(1e-5), f(0.1), p, p, p, p, p, need - 1, 0) == WORKSPACE and err() == "sd_bn_train_stats_bf16: workspace too small"
    assert lib.sd_col_sum(p, 4096, 64, p, 0, p, need - 1, 0) == WORKSPACE and err() == "sd_col_sum: workspace too small"
    assert lib.sd_bn_bwd(p, p, p, 0, 4096, 64, p, p, p, p, p, p, p, p, 0, p, need - 1, 0) == WORKSPACE and err() == "sd_bn_bwd: workspace too small"
    assert lib.sd_maxpool_bn_relu_bwd_bf16_dx16(p, p, p, 1, 64, 64, 64, p, p, p, p, p, p, p, 0, p, need - 1, 0) == WORKSPACE
    assert err() == "sd_maxpool_bn_relu_bwd_bf16_dx16: workspace too small"
    need = lib.sd_head_bwd_workspace_bytes(2, 64, 128, 8)
    assert lib.sd_head_bwd(p, p, p, p, p, p, 2, 64, 128, 8, 0, p, need - 1, 0) == WORKSPACE and err() == "sd_head_bwd: workspace too small"
    assert lib.sd_head_bwd_bf16(p, p, p, p, p, p, 2, 64, 128, 8, 0, p, need - 1, 0) == WORKSPACE and err() == "sd_head_bwd_bf16: workspace too small"
    # the bf16 stem tail on an odd map: before everything else in the fused form, after the workspace in the reduce form
    text = ": the bf16 form needs even Hi, Wi"
    assert lib.sd_maxpool_bn_relu_bwd_bf16(p, p, p, 1, 5, 4, 6, p, p, p, p, p, p, p, 0, p, 0, 0) == INVALID and err() == "sd_maxpool_bn_relu_bwd_bf16" + text
    assert lib.sd_maxpool_bn_relu_bwd_bf16_dx16(p, p, p, 1, 4, 5, 64, p, p, p, p, p, p, p, 0, p, ws, 0) == INVALID and err() == "sd_maxpool_bn_relu_bwd_bf16_dx16" + text
    assert lib.sd_maxpool_bn_relu_bwd_reduce_bf16(p, p, p, 1, 5, 5, 64, p, p, p, p, p, p, 0, p, p, 0, 0) == WORKSPACE
    assert lib.sd_maxpool_bn_relu_bwd_reduce_bf16(p, p, p, 1, 5, 5, 64, p, p, p, p, p, p, 0, p, p, ws, 0) == INVALID and err() == "sd_maxpool_bn_relu_bwd_reduce_bf16" + text
    assert lib.sd_maxpool_bn_relu_bwd_apply_bf16(p, p, p, 1, 5, 5, 64, p, p, p, p, p, p, 0) == INVALID and err() == "sd_maxpool_bn_relu_bwd_apply_bf16" + text
    # n % 4 != 0
    hyper = (f(1e-3), f(0.9), f(0.999), f(1e-8), f(1.0))
    assert lib.sd_cast_f32_to_bf16(p, p, 4098, 0) == INVALID and err() == "sd_cast_f32_to_bf16: bad arguments (n % 4 == 0, 16-byte aligned source)"
    assert lib.sd_cast_bf16_to_f32(p, p, 4098, 0) == INVALID and err().startswith("sd_cast_bf16_to_f32: bad arguments (n % 4 == 0")
    assert lib.sd_adam_step(p, p, p, p, 4098, 1, *hyper, 0) == INVALID and err() == "sd_adam_step: bad arguments (n % 4 == 0, step >= 1)"
    assert lib.sd_optim_step(p, p, p, p, 4098, 1, *hyper, f(0), 0, f(0), 0, 0, 0, f(0), 0, 0) == INVALID and err() == "sd_optim_step: bad arguments (n % 4 == 0, step >= 1)"
    assert lib.sd_grad_sumsq(p, 4098, p, ws, 0) == INVALID and err() == "sd_grad_sumsq: bad arguments (n % 4 == 0)"
    # the caller-provided-rows forms keep their two texts
    assert lib.sd_bn_finalize_stats(p, 0, 64, 64, f(1e-5), f(0.1), p, p, p, p, 0, 0) == INVALID and err() == "sd_bn_finalize_stats: bad arguments"
    assert lib.sd_bn_bwd_finalize(p, 8, 64, 64, p, p, 0, 0, 0, 0) == INVALID and err() == "sd_bn_bwd_finalize: bad arguments"
    assert lib.sd_bn_stats_sums(p, 8, 64, 64, 0, 0, 0) == INVALID and err() == "sd_bn_stats_sums: bad arguments (null pointer or rows <= 0)"
    assert lib.sd_bn_bwd_sums(p, 8, 64, 64, p, 0, 0, p, 0, 0) == INVALID and err() == "sd_bn_bwd_sums: bad arguments (null pointer or rows <= 0)"
    assert lib.sd_bn_train_sums_bf16(p, 64, 64, 0, p, ws, 0) == INVALID and err() == "sd_bn_train_sums_bf16: null sums"
    assert lib.sd_upsample2x_bwd_bf16(p, 0, p, 1, 2, 2, 6, 0) == INVALID and err() == "sd_upsample2x_bwd_bf16: bad arguments"
    assert lib.sd_bn_relu_maxpool_fwd(p, 1, 4, 4, 6, p, p, p, p, p, p, 0) == INVALID and err() == "sd_bn_relu_maxpool_fwd: bad arguments"


def threshold_grid():
    """M around every threshold of red_rows (M / r crosses 1024 for r = 256 .. 32) and of fold_rows (more than 2048 partial rows; the slab
    max(16, rows / 128) grows from 16 to 17 at 2176 rows)."""
    edges = [1, 16, 1024 * 16] + [1024 * r for r in (32, 64, 128, 256)] + [2048 * 256, 2176 * 256, 4096 * 256]
    return sorted({max(1, e + k) for e in edges for k in (-257, -256, -255, -17, -16, -15, -1, 0, 1, 15, 16, 17, 255, 256, 257)})


def test_size_queries_equal_the_plan_around_every_threshold(lib):
    zero = dict.fromkeys(TOOL.DESC_FIELDS, 0)
    for M in threshold_grid():
        for C_ in (4, 64, 512, 1024):
            want = R.plan(M, C_)
            assert lib.sd_col_reduce_workspace_bytes(M, C_) == want.workspace_bytes, (M, C_)
            _, plan = parse(ask(lib, dict(zero, op=OP["bn_train_stats"], M=M, C=C_)))
            assert (plan["rpb"], plan["nb"], plan["ws_bytes"]) == (want.rpb, want.nb, want.workspace_bytes), (M, C_)
            assert (plan["slab"], plan["rows"]) == ((want.fold.slab, want.fold.rows_out) if want.fold else (0, want.nb)), (M, C_)
        # the head's partial rows: one per 1024 pixels, or one per wave of the C = 128 kernel (up to 1024, a multiple of four)
        for C_, Co in ((128, 8), (64, 5), (256, 32)):
            rows = max(R.cdiv(M, 1024), min(1024, (R.cdiv(M, 16) + 3) // 4 * 4))
            want = (rows * (Co * C_ + Co) * 4 + 255) // 256 * 256
            assert lib.sd_head_bwd_workspace_bytes(1, M, C_, Co) == want, (M, C_, Co)
            if M < 1 << 22:
                _, plan = parse(ask(lib, dict(zero, op=OP["head_bwd"], B=1, H=M, C=C_, Co=Co, flags=15)))
                assert plan["ws_bytes"] == want
    for rows in (1, 2047, 2048, 2049, 2175, 2176, 2177, 8192, 100000):
        assert lib.sd_bn_finalize_scratch_rows(rows) == R.fold_rows(rows)
        for C_, scratch in ((64, True), (64, False), (512, True), (1024, True)):
            fold = R.fold_plan(rows, C_, scratch)
            _, plan = parse(ask(lib, dict(zero, op=OP["bn_finalize_stats"], M=rows * 16, C=C_, rows=rows, flags=TOOL.F_SCRATCH if scratch else 0)))
            assert (plan["slab"], plan["rows"]) == ((fold.slab, fold.rows_out) if fold else (0, rows)), (rows, C_, scratch)
