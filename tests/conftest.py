import os
import sys

import pytest

# torch first, before any test loads libvolym_hip.so: torch ships its own HIP and HSA runtimes, and its libraries ask for
# them under names (libamdhip64.so, libhsa-runtime64.so) that do not match the ROCm ones libvolym_hip.so already pulled
# in, so loading the library first puts two runtimes in one process -- torch then sees no device and RCCL (torch's
# librccl.so.1, which the library dlopens) fails in ncclCommInitRank.  Imported first, torch's runtimes are the
# process's only ones, as in bench.py.
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run through gpurun)")


@pytest.fixture(scope="session")
def oracle():
    """The CPU oracle (test infrastructure; built on demand with gcc)."""
    from oracle import oracle as O
    O.lib()
    return O


@pytest.fixture(scope="session")
def volym_lib():
    """libvolym_hip.so; built on demand (hipcc cross-compiles without a GPU)."""
    from volym_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()
