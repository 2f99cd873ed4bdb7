"""Every entry point of the BatchNorm / pool / head / optimizer host layer (the tail of csrc/sd_nn.hip) returns and writes exactly what
tests/golden/nn_call_trace.json records: per call of tools/nn_trace.py the return code, the error text of a refusal, the SHA-256 (first
digits) of every output buffer and of the workspace, and the answers of the size queries.  The fixture is written by `tools/nn_trace.py`
on a checkout of the commit this layer must stay equal to, never on the code under test."""
import importlib.util
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _tool():
    spec = importlib.util.spec_from_file_location("nn_trace", ROOT / "tools" / "nn_trace.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


TOOL = _tool()


def test_every_call_returns_and_writes_what_the_recorded_one_did():
    recorded = {c["name"]: c for c in TOOL.load_fixture()["calls"]}
    calls = TOOL.run_calls()
    assert sorted(c["name"] for c in calls) == sorted(recorded) and len(calls) == len(recorded)
    differing = []
    for got in calls:
        want = recorded[got["name"]]
        for key in ("desc", "rc", "error", "out", "sizes"):
            if got.get(key) != want.get(key):
                differing.append(f"{got['name']}: {key} = {got.get(key)!r}, recorded {want.get(key)!r}")
    assert not differing, f"{len(differing)} differences, the first ones:\n" + "\n".join(differing[:10])
