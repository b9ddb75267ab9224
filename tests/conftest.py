import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="session")
def gpu_present():
    """Whether torch sees a GPU, asked in a child process.  torch carries a HIP runtime of its own; loaded after the
    library's and initialised in this process, it takes the device, and the library's runtime finds none for the rest
    of the session."""
    import subprocess
    p = subprocess.run([sys.executable, "-c", "import torch; print(int(torch.cuda.is_available()))"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.strip().splitlines()[-1] == "1"


def pytest_sessionfinish(session, exitstatus):
    """The GPU parity tests record how much of each tolerance they used (tests/_tol.py)."""
    try:
        import _tol
        _tol.dump(os.path.join(ROOT, "gpurun_out", "tolerances_observed.json"))
    except Exception:
        pass
