import os
import sys
from pathlib import Path

import pytest

# torch's CPU exp (the oracle's Gaussian targets) runs through MKL VML, whose result bits depend on the code branch MKL picks for the
# host CPU: the goldens were produced on MKL's AVX-512 branch, while on a non-Intel host MKL takes its generic branch and some values
# move by one ulp.  Pinning the branch (read by MKL at its first call, before any test runs) makes the oracle host-independent.
os.environ.setdefault("MKL_CBWR", "AVX512")

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / "tests" / "golden"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
