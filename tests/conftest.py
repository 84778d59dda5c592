import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The suite runs with the hardware queues the package asks for on import (24: eight batches in flight, lane adoption on).
# The package leaves a GPU_MAX_HW_QUEUES already in the environment alone, so one inherited from the caller would
# otherwise decide the overlap depth of every test; nothing has started HIP yet when this file is read.
os.environ["GPU_MAX_HW_QUEUES"] = "24"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run via gpurun)")


@pytest.fixture(scope="session")
def oracle():
    from oracle import oracle as orc
    orc.build()
    return orc
