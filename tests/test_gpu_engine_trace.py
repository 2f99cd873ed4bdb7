"""The network engine hands the device exactly the launches recorded in tests/golden/engine_launch_trace.json: for every eval and
training schedule (tools/engine_trace.py CONFIGS) the same C-ABI calls in the same order, each with the same descriptor fields,
flags, modes, scalar arguments and null / non-null buffers.  The fixture is written by `tools/engine_trace.py record` on a checkout
of the commit the engine must stay equal to; `tools/engine_trace.py diff` lists every differing call."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _tool():
    spec = importlib.util.spec_from_file_location("engine_trace", ROOT / "tools" / "engine_trace.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


TOOL = _tool()


@pytest.fixture(scope="module")
def recorded():
    return json.loads(TOOL.FIXTURE.read_text())


def test_every_configuration_is_recorded(recorded):
    assert sorted(recorded) == sorted(TOOL.CONFIGS)


@pytest.mark.parametrize("name", list(TOOL.CONFIGS))
def test_engine_launch_trace_equals_the_recorded_one(name, recorded, tmp_path):
    lines, _ = TOOL.run_config(name)
    diff = TOOL.first_difference(lines, recorded[name])
    if diff is not None:
        out = tmp_path / f"{name}.txt"
        out.write_text("\n".join(lines) + "\n")
        pytest.fail(f"{name}: {len(lines)} calls, {recorded[name]['calls']} recorded; first difference at call {diff[0]}: {diff[1]} "
                    f"(full trace: {out}; `tools/engine_trace.py diff` lists the rest)")
    got = TOOL.summary(lines)
    assert got["calls"] == recorded[name]["calls"] and got["symbols"] == recorded[name]["symbols"] and got["sha256"] == recorded[name]["sha256"]
    # the mixed-precision step takes the bf16 stem (H % 32 == 0: the stem map is even), never the bf16-product / fp32-map one
    if name.startswith("train_amp"):
        assert not any(s.endswith("_bf16mm") and "stem_fwd" in s for s in got["symbols"])
        assert any(s.startswith("sd_conv2d_stem_fwd_bn_") and s.endswith("_bf16") for s in got["symbols"])
