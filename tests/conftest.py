import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cognitive-radio-network_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "gpu_first: a GPU test whose rank processes share the box's one GPU: runs before this "
                                       "process opens the device itself (see pytest_collection_modifyitems)")


def pytest_collection_modifyitems(config, items):
    """The multi-rank rehearsals of BASELINE.json configs[4] put several rank processes on the one GPU and gather in lock step over the
    stand-in wire.  A further process holding the device — this pytest process, once any in-process GPU test has run — competes with
    them for it: with eight ranks, where the driver hands compute queues to 8 processes at a time (amdgpu hws_max_conc_proc), every
    lock-step gather waited a scheduling round, 3.9 s -> 43 s for the same command (profiles/r06_nine_gpu_processes.txt); and the
    number of processes that may hold one GPU at once is capped.  So those tests go first, whatever files or -k expression selected
    them: at that point this process has made no GPU call."""
    first = [it for it in items if it.get_closest_marker("gpu_first")]
    if first:
        items[:] = first + [it for it in items if not it.get_closest_marker("gpu_first")]


@pytest.fixture(scope="session")
def built():
    """Make sure libcrnsense.so and the oracle exist (build() cross-compiles without a GPU)."""
    import __graft_entry__ as g
    lib = os.path.join(ROOT, "cognitive-radio-network_amd", "libcrnsense.so")
    orc = os.path.join(ROOT, "oracle", "libcrn_oracle.so")
    if not (os.path.exists(lib) and os.path.exists(orc)):
        g.build()
    return True
