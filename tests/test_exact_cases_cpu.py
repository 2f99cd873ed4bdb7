"""The inputs of the bit-exact conv / head tests (tests/test_gpu_exact.py) checked on the CPU: every case meets the exactness bound (all
partial sums are integers below 2^24, so fp32 arithmetic is exact in any order), every bf16 case has enough outputs that need rounding, are
exact ties, or round differently under truncation -- and the cases reach every kernel the dispatch plan can name.  Loads the library, makes
no HIP call."""
import ctypes as C
import importlib.util
from pathlib import Path

import pytest
import torch

from tests import helpers as X

ROOT = Path(__file__).resolve().parent.parent
REGIMES = ("round", "wide_a", "wide_b")


def _geoms(passes):
    seen = []
    for geom, _, names in X.EXACT_CONV_CASES:
        if any(p in names for p in passes) and geom not in seen:
            seen.append(geom)
    return seen


def test_bf16_rounding_helpers_are_nearest_even_and_truncation():
    g = torch.Generator().manual_seed(0)
    t = torch.cat([torch.randn(50000, generator=g) * 1000, torch.randint(-5000, 5000, (50000,), generator=g).float(),
                   torch.tensor([257.0, 259.0, 258.0, 1028.0, 1036.0, -257.0, 0.0, 1.5])])
    assert torch.equal(X.bf16_rne(t), t.bfloat16().float())
    assert torch.equal(X.bf16_rne(torch.tensor([257.0, 259.0, 1028.0, 1036.0, -257.0])), torch.tensor([256.0, 260.0, 1024.0, 1040.0, -256.0]))
    assert torch.equal(X.bf16_trunc(torch.tensor([257.0, 259.0, -259.0])), torch.tensor([256.0, 258.0, -258.0]))
    assert X.rounding_shares(torch.tensor([256.0, 257.0, 258.5, 259.0])) == (0.75, 0.5, 0.25)


def test_case_tables_stay_within_the_reference_budget():
    """every reference costs at most 2^31 multiply-adds, except the one geometry that the 256-row tile kernel's plan needs"""
    over = [g for g, _, _ in X.EXACT_CONV_CASES if X.conv_macs(g) > X.MAX_REFERENCE_MACS]
    assert set(over) == {X.BIG_TILE_CASE}
    for g in X.EXACT_SB_CASES + X.EXACT_WGRAD_BF16_CASES + [c[0] for c in X.EXACT_STATS_CASES] + [c[0] for c in X.EXACT_BNRED_CASES]:
        assert X.conv_macs(g) <= X.MAX_REFERENCE_MACS


@pytest.mark.parametrize("geom", _geoms((0, 16)) + X.EXACT_SB_CASES, ids=lambda g: "x".join(map(str, g)))
def test_forward_inputs_are_exact_and_round(geom):
    bf16 = geom[3] % 64 == 0
    for regime in REGIMES:
        if geom == X.BIG_TILE_CASE and regime != "round":
            continue
        p = X.fwd_problem(geom, regime)
        ref32 = X.assert_exact_reference(p["ref"], p["bound"], what=f"fwd {geom} {regime}")
        scale, shift, res = X.epilogue_operands(geom, geom[4], p["ref"].shape, wide=regime != "round")
        full = X.epilogue_ref(p["ref"], scale, shift, res, relu=True)
        X.assert_exact_reference(full, X.epilogue_bound(p["bound"], scale, shift, res), X.EXACT_LIMIT_HALVES, what=f"fwd epilogue {geom} {regime}")
        if regime == "round" and bf16:
            shares = X.assert_rounding_coverage(ref32, f"fwd {geom}")
            print(geom, "bound", float(p["bound"].max()), "shares", shares)


@pytest.mark.parametrize("geom", _geoms((1, 17)), ids=lambda g: "x".join(map(str, g)))
def test_data_gradient_inputs_are_exact_and_round(geom):
    for regime in REGIMES:
        p = X.dgrad_problem(geom, regime)
        ref32 = X.assert_exact_reference(p["ref"], p["bound"], what=f"dgrad {geom} {regime}")
        _, _, res = X.epilogue_operands(geom, geom[3], p["ref"].shape, salt=1, wide=regime != "round")
        X.assert_exact_reference(p["ref"] + res.double(), p["bound"] + res.double().abs(), what=f"dgrad + residual {geom} {regime}")
        if regime == "round":
            # a 1x1 / stride 2 data gradient is zero on three pixels of four: the shares are those of the pixels a tap reaches
            live = ref32[:, :, ::2, ::2] if geom[5] == 1 and geom[6] == 2 else ref32
            X.assert_rounding_coverage(live, f"dgrad {geom}")


@pytest.mark.parametrize("geom", _geoms((2,)) + X.EXACT_WGRAD_BF16_CASES, ids=lambda g: "x".join(map(str, g)))
def test_weight_gradient_inputs_are_exact(geom):
    for regime in REGIMES:
        p = X.wgrad_problem(geom, regime)
        X.assert_exact_reference(p["ref"], p["bound"], what=f"wgrad {geom} {regime}")
        base = X.int_uniform(torch.Generator().manual_seed(5), p["ref"].shape, 2047)
        X.assert_exact_reference(p["ref"] + base.double(), p["bound"] + base.double().abs(), what=f"wgrad accumulate {geom} {regime}")


@pytest.mark.parametrize("shape", X.EXACT_STEM_SHAPES)
def test_stem_inputs_are_exact_and_round(shape):
    for regime in REGIMES + ("stats",):
        p = X.stem_problem(shape, regime)
        ref32 = X.assert_exact_reference(p["ref"], p["bound"], what=f"stem {shape} {regime}")
        if regime == "round":
            X.assert_rounding_coverage(ref32, f"stem {shape}")
        if regime == "stats":
            assert float((p["ref"] ** 2).sum((0, 2, 3)).max()) < X.EXACT_LIMIT
    g = (shape[0], shape[1], shape[2], 3, 64, 7, 2, 3)
    for regime in REGIMES:
        p = X.wgrad_problem(g, regime)
        X.assert_exact_reference(p["ref"], p["bound"], what=f"stem wgrad {shape} {regime}")


@pytest.mark.parametrize("entry", X.EXACT_STATS_CASES, ids=X.case_id)
def test_statistics_inputs_keep_the_sums_of_squares_exact(entry):
    geom = entry[0]
    p = X.fwd_problem(geom, "stats")
    ref32 = X.assert_exact_reference(p["ref"], p["bound"], what=f"stats {geom}")
    assert float((p["ref"] ** 2).sum((0, 2, 3)).max()) < X.EXACT_LIMIT
    y16 = X.bf16_rne(ref32).double()
    assert float((y16 ** 2).sum((0, 2, 3)).max()) < X.EXACT_LIMIT and float(y16.abs().sum((0, 2, 3)).max()) < X.EXACT_LIMIT


@pytest.mark.parametrize("case", X.EXACT_HEAD_CASES + X.EXACT_HEAD_BF16_BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_inputs_are_exact(case):
    for regime in REGIMES:
        p = X.head_problem(case, regime)
        for k in ("y", "dx", "dw", "db"):
            X.assert_exact_reference(p[k], p[k + "_bound"], what=f"head {case} {regime} {k}")
    p = X.head_problem(case, "round")
    assert float(p["w"].abs().max()) <= 256 and torch.equal(p["w"].bfloat16().float(), p["w"])     # hi / lo bf16 split: lo = 0
    if case in X.EXACT_HEAD_BF16_BWD_CASES:                     # sd_head_bwd_bf16 stores dx as bf16
        X.assert_rounding_coverage(p["dx"].float(), f"head dx {case}")


def _names(lib, L, geom, opts, passes):
    with X.dispatch_options(lib, opts):
        d = X.conv_desc(L, geom)
        return {p: lib.sd_conv2d_kernel_name(C.byref(d), p).decode() for p in passes}


def test_every_case_names_the_kernel_the_plan_picks():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    for geom, opts, names in X.EXACT_CONV_CASES:
        assert set(opts) <= set(X.OPTION_DEFAULTS)
        assert _names(lib, L, geom, opts, names) == names, (geom, opts)
    for geom, opts, names in X.EXACT_STATS_CASES:
        assert _names(lib, L, geom, opts, names) == names, (geom, opts)
    for geom, opts, name in X.EXACT_BNRED_CASES:
        assert _names(lib, L, geom, opts, (1,)) == {1: name}, (geom, opts)


def test_exact_cases_reach_every_kernel_of_the_dispatch_plan():
    """tools/conv_dispatch_table.py sweeps descriptors and options over the plan (plan_conv / plan_wgrad): every kernel name it yields must
    be reached by an exact case under the options that case sets -- a kernel added to the plan later is either tested or flagged here."""
    from structuredetector_amd import _lib as L
    spec = importlib.util.spec_from_file_location("conv_dispatch_table", ROOT / "tools" / "conv_dispatch_table.py")
    table = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(table)
    assert table.DEFAULTS == X.OPTION_DEFAULTS
    swept = {n for line in table.table(L) for n in eval(line)[8:13]}
    assert len(swept) >= 37
    lib = L.lib()
    reached = set()
    for geom, opts, names in X.EXACT_CONV_CASES:
        reached |= set(_names(lib, L, geom, opts, names).values())
    missing = sorted(swept - reached)
    assert not missing, f"kernels of the dispatch plan that no exact case reaches: {missing}"
    # the options are back at their defaults
    d = X.conv_desc(L, (2, 32, 32, 128, 128, 3, 1, 1))
    assert lib.sd_conv2d_kernel_name(C.byref(d), 0).decode() == "k_conv_igemm<128, 0, false>"
