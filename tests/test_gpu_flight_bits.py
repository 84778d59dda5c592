"""The flight kernels return the bits recorded in tests/golden/flight_bits_*.npy: no tolerance.

The files were recorded by tools/record_flight_bits.py on the commit before the fp64 throughput RK4 step was shortened (dead
register copies of polynomial coefficients, LDS records addressed by byte offset, the step counter taken out of the step): a
change of that kind may not alter what any floating-point instruction computes, in any of the three builds.  Batches and calls are those of
flight_bits_cases.py: the four specialisations the launcher picks (wind table or none, liquid or solid motor) on 256
Set S samples with the full termination logic, a planar CSV-wind batch flown to the ground under the parachute, the
trajectory-capture build with four captured samples, and the steered groups of flight_event_cases.py which end in every way the event
logic knows (recorded later, on the commit that added them: its only kernel change is the record count the capture instantiation
reports for a flight whose loop is never entered, which none of these cases captures - the older files did not change)."""
import os

import numpy as np
import pytest
import torch

import flight_bits_cases as cases
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


def golden(case, precision, name):
    path = os.path.join(H.GOLDEN, cases.file_name(case, precision, name))
    assert os.path.getsize(path) <= 256 * 1024
    return np.load(path)


@pytest.mark.parametrize("precision", cases.PRECISIONS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_the_recording_has_every_way_a_flight_ends(case, precision):
    flight = golden(case, precision, "flight")
    assert flight.shape == (17, cases.CASES[case][2]) and flight.dtype == np.float64
    assert cases.missing_ends(case, flight) == []


@pytest.mark.parametrize("precision", cases.PRECISIONS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_same_bits_as_recorded(engine, case, precision):
    got = cases.collect(engine, case, precision)
    for name, a in got.items():
        want = golden(case, precision, name)
        same = np.array_equal(a, want, equal_nan=True)
        if not same and a.shape == want.shape:
            bad = np.argwhere(~((a == want) | (np.isnan(a) & np.isnan(want))))
            print("%s %s %s: %d of %d values differ, first at %s: %r != %r" % (
                case, precision, name, len(bad), a.size, bad[0].tolist(), a[tuple(bad[0])], want[tuple(bad[0])]))
        assert same, (case, precision, name)
