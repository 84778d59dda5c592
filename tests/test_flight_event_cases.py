"""The steered batch of flight_event_cases.py does what the GPU tests rely on: on the CPU oracle every class of ending is
populated, healthy and far enough from every threshold of the event logic that no build can change a sample's class by
rounding.  (The fp32 build is held to 0.1 % on the first apogee; the margins here are 1 %.)"""
import numpy as np
import pytest

from erpl_monte_carlo_sim_amd import _abi

import flight_event_cases as ev


@pytest.fixture(scope="module")
def runs(oracle):
    """[(group, summary, status, classes, counted mask), ...] on the oracle."""
    out = []
    for g in ev.groups():
        summ, status = oracle.run_batch(ev.config(g.name), g.hb, flags=g.flags)
        out.append((g, summ, status) + ev.counted(summ, status, g.flags))
    return out


def test_sizes_and_inputs():
    gs = ev.groups()
    assert len(gs) == len(ev.SPECS) and sum(g.hb.n for g in gs) == ev.N_SAMPLES <= 512
    assert all(g.hb.n <= 128 for g in gs)
    assert any(g.kind == "solid" for g in gs)
    for g in gs:   # one sample replicated: everything but the steered rows is the same in every column
        assert np.all(g.hb.ic == g.hb.ic[:, :1]) and np.all(g.hb.wind == g.hb.wind[:, :, :1])
        assert np.all(g.hb.motor[1:3] == g.hb.motor[1:3, :1])
        assert ev.config(g.name).max_time <= 300.0


def test_every_class_is_populated_and_healthy(runs):
    count = dict.fromkeys(ev.CLASSES, 0)
    tiers = {300: 0, 120: 0, 60: 0}
    dropped = 0
    for g, summ, status, cls, ok in runs:
        dropped += int(np.sum(~ok))
        for c in cls[ok]:
            count[c] += 1
        for t in ev.tier(summ)[ok & (cls == "apogee_stop")]:
            tiers[int(t)] += 1
        print("%-10s n %3d  counted %3d  %s" % (g.name, g.hb.n, ok.sum(), {c: int(np.sum(cls[ok] == c)) for c in sorted(set(cls[ok]))}))
    print("oracle class counts:", count, " apogee_stop by coast limit:", tiers, " left out:", dropped, "of", ev.N_SAMPLES)
    assert all(v >= 3 for v in count.values()), count
    assert all(v >= 3 for v in tiers.values()), tiers
    assert dropped <= 0.10 * ev.N_SAMPLES
    # none of them comes near what makes the fp64 throughput build hand a lane to the reference-order kernel (1e6 m/s,
    # 100 km below the pad): every counted flight is integrated by the build it is submitted to
    for g, summ, status, cls, ok in runs:
        assert np.all(summ[_abi.SUM_MAX_SPEED][ok] < 1e4) and np.all(summ[_abi.SUM_IMPACT_Z][ok] > -1e4)
    solid = {c for g, _, _, cls, ok in runs if g.kind == "solid" for c in cls[ok]}
    assert {"coast_60", "altitude_unlatched"} <= solid


def test_no_sample_sits_near_a_threshold(runs):
    """1 % on the first apogee against the latch threshold and the three limits; a coast-out still 1 % above the 25 km it
    needs; a flight that ran out of time clear of the ground.  An altitude exit cannot be 1 % away from 100 km - it ends on
    the first step above it - so that class is held to what the margin stands for instead: its vertical speed at the exit
    would have carried it more than 1 % (1000 m) further, vz^2 / 2g > 1000 m at g < 9.81 m/s^2."""
    for g, summ, status, cls, ok in runs:
        fa = summ[_abi.SUM_FIRST_APOGEE_ALT][ok]
        out = cls[ok] == "altitude_unlatched"
        for edge in (1000.0, 25000.0, 50000.0, 100000.0):
            near = np.abs(fa - edge) <= 0.01 * edge
            if edge == 100000.0:
                near &= ~out
            assert not np.any(near), (g.name, edge, fa[near])
        vz = summ[_abi.SUM_FINAL_VZ][ok][out]
        assert np.all(vz * vz / (2 * 9.81) > 1000.0), (g.name, vz)
        z = summ[_abi.SUM_IMPACT_Z][ok]
        coast = np.isin(cls[ok], ("coast_60", "coast_120"))
        assert np.all(z[coast] > 25250.0), (g.name, z[coast])
        timed = np.isin(cls[ok], ("max_time_ascent", "max_time_latched"))
        assert np.all(z[timed] > 1.0), (g.name, z[timed])


def test_coast_outs_end_one_limit_after_their_apogee(runs):
    """flight_time - first_apogee_time = 60 s + k dt (first apogee above 50 km) or 120 s + k dt (25 to 50 km), 0 < k <= 3:
    the class is tied to the limit that ended the flight, not only to the altitude."""
    seen = 0
    for g, summ, status, cls, ok in runs:
        dt = min(ev.config(g.name).dt_initial, 0.005)      # simulator.py:209
        for name, limit in (("coast_60", 60.0), ("coast_120", 120.0)):
            m = ok & (cls == name)
            over = (summ[_abi.SUM_FLIGHT_TIME] - summ[_abi.SUM_FIRST_APOGEE_TIME])[m] - limit
            assert np.all((over > -1e-9) & (over <= 3 * dt + 1e-9)), (g.name, name, over)
            assert np.all(ev.tier(summ)[m] == limit)
            seen += int(m.sum())
    assert seen >= 6
