import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP device)")
    config.addinivalue_line("markers", "slow: long-running test")


def gpu_available() -> bool:
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="session")
def native():
    import uda_amd
    return uda_amd.native()


@pytest.fixture
def sock_dir():
    """A short directory for Unix socket files: sockaddr_un.sun_path holds 107 bytes, and pytest's
    tmp_path under a deep TMPDIR is longer than that."""
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="uda-", dir="/tmp")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session")
def require_gpu():
    if not gpu_available():
        pytest.fail("GPU test collected on a machine without a HIP device")
