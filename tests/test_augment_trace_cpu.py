"""The augmentation policy layer (data/augment.py ValidationAugmentation / TrainAugmentation, the flag checks of utils/args.py) does what
tests/golden/augment_call_trace.json records of the commit it must stay equal to: for every configuration of tools/augment_trace.py the
same calls into `preprocess_images` / `preprocess_image_list` / `transpose_select` with the same host tables, the same annotations and
the same generator state afterwards (the fixture keeps names and sizes in the clear and every table behind a digest of its full text); the same descriptors out of `_chain_desc`; the same answers of the flag checks.  The fixture is
written by `tools/augment_trace.py record` on a checkout of that commit; `tools/augment_trace.py diff` lists every differing entry."""
import importlib.util
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _tool():
    spec = importlib.util.spec_from_file_location("augment_trace", ROOT / "tools" / "augment_trace.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


TOOL = _tool()


@pytest.fixture(scope="module")
def recorded():
    return json.loads(TOOL.FIXTURE.read_text())


def _same(part, got, want):
    diff = TOOL.differences(TOOL.brief(part, got), want)
    assert not diff, "\n".join(diff[:20]) + "\n(`tools/augment_trace.py diff --dump DIR` on both checkouts shows the tables)"


def test_every_configuration_and_descriptor_case_is_recorded(recorded):
    assert sorted(recorded["configs"]) == sorted(TOOL.CONFIGS)
    assert sorted(recorded["descriptors"]) == sorted(name for name, _, _ in TOOL.DESC_CASES)
    assert len(recorded["flags"]) == 1 + 2 * sum(len(v) for v in TOOL.FLAG_PROBES.values())


@pytest.mark.parametrize("name", list(TOOL.CONFIGS))
def test_call_trace_annotations_and_generator_state_equal_the_recorded_ones(name, recorded):
    got = TOOL.trace_config(name)
    _same("configs", got, recorded["configs"][name])
    if name.startswith("refuse_"):
        assert got["error"][0] == "SdError" and not got["calls"]
    elif name.startswith("everything"):                              # two size groups: two chain calls and one transpose
        assert [c["fn"] for c in got["calls"]] == ["preprocess_images", "preprocess_images", "transpose_select"]


def test_chain_descriptors_equal_the_recorded_ones(recorded):
    got = TOOL.trace_descriptors()
    for name, entry in got.items():
        _same("descriptors", entry, recorded["descriptors"][name])
    every = got["window_all"]["tables"]
    assert every["affine"] is None and all(v is not None for k, v in every.items() if k != "affine")
    assert [got[f"{g}_plain"]["scalars"]["geometry"] for g in ("stretch", "window", "letterbox")] == [0, 1, 2]


def _probes(row):
    """The values one row of the flag table is asked about: both ends (of a half-open range the open end, which is refused, and a value
    just below it), just outside them, NaN, True and a value inside; for a range that starts above 0 also 0 (= off) and a float."""
    lo, hi, mid = type(row.default)(row.lo), type(row.default)(row.hi), type(row.default)((row.lo + row.hi) / 2)
    if row.integer:
        return [0, lo, hi, lo - 1, hi + 1, -1, float("nan"), True, mid, float(mid)]
    return [lo, hi, round(lo - 0.001, 3), round(hi - 0.001, 3) if row.open_hi else round(hi + 0.001, 3), float("nan"), True, mid]


def _flag_rows():
    from structuredetector_amd.utils.args import AUG_FLAGS
    return list(AUG_FLAGS.values())


@pytest.mark.parametrize("row", _flag_rows(), ids=lambda row: row.name)
def test_flag_checks_answer_as_recorded(row, recorded):
    """Walks the table: the default, the accepted ends, the refused neighbours, NaN, True, and every positive value under --synthetic,
    each compared with what the recorded commit's `check_aug_*`, `Trainer` checks, `finalize` and `TrainAugmentation` did with the same
    namespace (its quirks included: the two oldest checks take True as 1.0)."""
    from structuredetector_amd.utils.args import Arguments
    want = recorded["flags"]
    assert repr(getattr(Arguments().parser.parse_args([]), row.name)) == repr(row.default) == want["absent"]["parser"][row.name]
    for value in _probes(row):
        for synthetic in (0, 8):
            key = TOOL.probe_key(row.name, value, synthetic)
            assert key in want, f"{key}: the table's range is not the recorded commit's"
            got = TOOL.trace_flag(row.name, value, synthetic)
            _same("flags", got, want[key])
            inside = value == value and value is not True and (row.lo <= value <= row.hi and (value < row.hi or not row.open_hi) or value == 0)
            if not inside and value is not True:                     # outside and NaN: refused by the parser's validation and by train's check
                assert got["finalize"][0] == "AssertionError", key
                if "check" in got and row.name != "aug_transpose":   # (that check keeps its own logic: it asks for a square input only)
                    assert got["check"][0] == got["train"][0] == "ValueError" and "should be" in got["check"][1], key
            if inside and not (row.integer and isinstance(value, float)):
                assert got["finalize"][0] == "RuntimeError", key     # (where a machine without a GPU stops: behind the last assert)
                refused = bool(row.source) and value > 0 and synthetic
                assert got["train"][0] == ("ValueError" if refused else "ok"), key
                if refused:
                    assert "source images" in got["train"][1] and "--synthetic" in got["train"][1], key


def test_a_namespace_from_before_the_flags_gives_their_defaults(recorded):
    got = TOOL.trace_absent()
    _same("flags", got, recorded["flags"]["absent"])
    from structuredetector_amd.utils.args import AUG_FLAGS
    policy = dict(eval(got["policy"][1]))
    assert all(policy[name[4:]] == row.default for name, row in AUG_FLAGS.items())
