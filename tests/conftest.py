import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The CPU results the tests compare against (tests/golden/, the reference records) were computed with 8 intra-op threads.  ATen's
# CPU kernels split their reductions by the thread count, so another count sums in another order and misses the 2e-6 bars of the
# fixture tests.  Every test process, and every child process a test starts, runs with that count whatever the host has.
CPU_THREADS = 8
os.environ["OMP_NUM_THREADS"] = os.environ["MKL_NUM_THREADS"] = str(CPU_THREADS)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `pytest -m gpu` on the GPU box)")
    import torch
    torch.set_num_threads(CPU_THREADS)


def golden_path(name: str) -> str:
    return os.path.join(ROOT, "tests", "golden", name.replace("+", "p") + ".npz")


@pytest.fixture(scope="session")
def amd_lib():
    from oracle import cases
    return cases.lib_namespace("amd")
