"""The statistics calls return the bits recorded in tests/golden/stats_bits.json: no tolerance.

The file was recorded by tools/record_stats_bits.py on the commit before the reductions of erpl_analysis.hip,
erpl_distributions.hip and erpl_correlation.hip moved into erpl_stat_device.h.  The last bit of every sum and the sign of
a zero minimum depend on the order of the reduction, so equality here pins that order: inputs and calls are those of
stats_bits_cases.py (rows of standard_normal * 10**uniform(-3, 6), NaN and +-inf planted, one non-negative row with +0.0
near its front and -0.0 near its end), at the smallest sizes that reach every level of the fold.

tests/golden/stats_host_bits.json does the same for bootstrap and impact_density (collect_host_size), recorded with
`tools/record_stats_bits.py --host` on the commit before their host halves moved onto the layouts of
csrc/erpl_stat_layout.h: every branch of the two entry points, and at 262 444 samples the one density call with several
source slices and partial sums near the bound of their piece."""
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
import stats_bits_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats_bits.json")
HOST_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats_host_bits.json")


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(GOLDEN) <= 64 * 1024
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def host_golden():
    assert os.path.getsize(HOST_GOLDEN) <= 64 * 1024
    with open(HOST_GOLDEN) as f:
        return json.load(f)


def differences(got, want, path=""):
    """Every leaf at which two JSON trees differ, as 'path: got != want'."""
    if isinstance(want, dict) or isinstance(got, dict):
        if not (isinstance(want, dict) and isinstance(got, dict)) or set(got) != set(want):
            return [f"{path}: keys differ"]
        return [d for k in sorted(want) for d in differences(got[k], want[k], f"{path}/{k}")]
    if isinstance(want, list) or isinstance(got, list):
        if not (isinstance(want, list) and isinstance(got, list)) or len(got) != len(want):
            return [f"{path}: lengths differ"]
        return [d for k in range(len(want)) for d in differences(got[k], want[k], f"{path}[{k}]")]
    return [] if got == want and type(got) is type(want) else [f"{path}: {got} != {want}"]


def test_the_recording_covers_the_sizes(golden):
    assert sorted(golden) == sorted(str(n) for n in cases.SIZES)
    assert "correlation_wide" in golden[str(cases.WIDE_CORR_N)]


@pytest.mark.parametrize("n", [n for n in cases.SIZES if n >= 65])
def test_inputs_can_tell_summation_orders_apart(n):
    summ, fac, mask, _ = cases.make_inputs(n)
    for k, x in enumerate(cases.rows_used(n, summ, fac)):
        assert cases.order_sensitive(x), k
    zero = summ[cases.ZERO_ROW]
    fin = zero[np.isfinite(zero)]
    assert fin.min() == 0.0 and not np.signbit(zero[3]) and np.signbit(zero[n - 2]) and mask[3] == 0 and mask[n - 2] == 0
    assert 0.05 < np.count_nonzero(mask) / n < 0.2


@pytest.mark.parametrize("n", cases.SIZES)
def test_same_bits_as_recorded(engine, golden, n):
    got = json.loads(json.dumps(cases.collect_size(engine, n)))
    diff = differences(got, golden[str(n)], f"n={n}")
    assert not diff, "\n".join(diff[:40])


def test_the_host_recording_covers_the_sizes_and_branches(host_golden):
    assert sorted(host_golden) == sorted(str(n) for n in cases.HOST_SIZES)
    assert set(host_golden["1"]) == {"bootstrap", "density"}
    assert set(host_golden["65"]) == {"bootstrap", "bootstrap_empty", "density", "density_flat"}
    assert set(host_golden["1025"]) == {"bootstrap", "bootstrap_extra_alone", "density", "density_no_samples", "density_explicit"}
    assert set(host_golden[str(cases.HOST_SIZES[-1])]) == {"density"}
    assert host_golden["65"]["bootstrap_empty"]["count"] == 0 and not host_golden["65"]["density_flat"]["solid"]
    assert all(host_golden[str(n)]["density"]["solid"] for n in cases.HOST_SIZES[1:])
    assert host_golden[str(cases.HOST_SIZES[-1])]["density"]["count"] > 200000


@pytest.mark.parametrize("n", cases.HOST_SIZES)
def test_same_host_bits_as_recorded(engine, host_golden, n):
    got = json.loads(json.dumps(cases.collect_host_size(engine, n)))
    diff = differences(got, host_golden[str(n)], f"n={n}")
    assert not diff, "\n".join(diff[:40])
