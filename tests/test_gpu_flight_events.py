"""Every way a flight ends, in all three builds, against the CPU oracle (run on a real MI355X: `pytest -m gpu`).

The batches are the steered groups of flight_event_cases.py; test_flight_event_cases.py shows on the oracle that they populate
every class of ending with a 1 % margin to every threshold of the event logic.  Only the classified, healthy samples are compared.
The bars are those of test_gpu_parity.py:
  fp64 reference order : test_cfg2_set_p_to_apogee_fp64 - the whole status word, step count and the three times equal, 1e-9 on first
                         apogee / apogee / max speed, 1e-7 on the range
  fp64 throughput      : test_randomised_configurations - status, steps, rail-exit time equal, 1e-8 on the same four rows
  fp32                 : 0.1 % on the first apogee and 25 steps where the ending is decided no later than the latch; the same 25 steps
                         on the time a coast-out spends between its apogee and its end; the landings after a descent are chaotic in
                         fp32 (test_fp32_full_flight_landing) and only reported.
Then the launch structure (order, neighbours, step chunks, lane adoption, refill) must not change a bit of any of it, and the
trajectory-capture instantiation must write the oracle's records."""
import functools

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, flatten, models

import flight_event_cases as ev
import helpers as H

pytestmark = pytest.mark.gpu

PRECISIONS = ("f64", "f64_fast", "f32")
EARLY = ("ground_step1", "altitude_unlatched", "max_time_ascent", "never_entered", "apogee_stop")   # decided no later than the latch
COAST = ("coast_60", "coast_120")
LATE = ("ground_unlatched", "ground_latched_chute", "stop_flag_never_latches", "max_time_latched")  # after a descent
ROWS = {"first apogee": _abi.SUM_FIRST_APOGEE_ALT, "apogee": _abi.SUM_APOGEE_ALT, "max speed": _abi.SUM_MAX_SPEED,
        "range": _abi.SUM_RANGE}
EXACT = {"steps": _abi.SUM_STEPS, "flight time": _abi.SUM_FLIGHT_TIME, "first apogee time": _abi.SUM_FIRST_APOGEE_TIME,
         "rail exit time": _abi.SUM_RAIL_EXIT_TIME}


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def ref(oracle):
    """{group name: (oracle summary, oracle status, classes, counted mask)}: computed once, read-only."""
    out = {}
    for g in ev.groups():
        summ, status = oracle.run_batch(ev.config(g.name), g.hb, flags=g.flags)
        out[g.name] = (summ, status) + ev.counted(summ, status, g.flags)
    return out


def fly(engine, g, precision, hb=None, submit=False, **kw):
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    engine.set_config(ev.config(g.name))
    db = DeviceBatch.from_host(g.hb if hb is None else hb, engine.device, _abi.PRECISIONS[precision])
    if submit:
        out = engine.submit(db, flags=g.flags, **kw)
        engine.wait()
        engine.synchronize()
    else:
        out = engine.run(db, flags=g.flags, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


_PLAIN = {}


def plain(engine, precision):
    """{group name: (summary, status)} of one build with the library's default launch: flown once per module, read-only."""
    if precision not in _PLAIN:
        _PLAIN[precision] = {g.name: fly(engine, g, precision) for g in ev.groups()}
    return _PLAIN[precision]


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(a - b) / np.abs(b)
    return np.where(a == b, 0.0, e)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_ending_matches_the_oracle(engine, ref, precision):
    got = plain(engine, precision)
    worst = dict.fromkeys(list(ROWS) + list(EXACT) + ["coast time"], 0.0)
    status_diff, counts, late = 0, {}, {}
    failures = []
    for g in ev.groups():
        (summ, status), (osum, ostat, cls, ok) = got[g.name], ref[g.name]
        dt = min(ev.config(g.name).dt_initial, 0.005)
        early, coast = ok & np.isin(cls, EARLY), ok & np.isin(cls, COAST)
        sel = ok if precision != "f32" else (early | coast)
        for c in cls[ok]:
            counts[c] = counts.get(c, 0) + 1
        bad = sel & (status != ostat)
        status_diff += int(bad.sum())
        if bad.any():
            failures.append((g.name, "status", np.flatnonzero(bad).tolist(), status[bad].tolist(), ostat[bad].tolist()))
        for name, row in ROWS.items():
            worst[name] = max(worst[name], float(np.max(relerr(summ[row], osum[row])[sel], initial=0.0)))
        for name, row in EXACT.items():
            worst[name] = max(worst[name], float(np.max(np.abs(summ[row] - osum[row])[sel], initial=0.0)))
        ct, oct_ = (s[_abi.SUM_FLIGHT_TIME] - s[_abi.SUM_FIRST_APOGEE_TIME] for s in (summ, osum))
        worst["coast time"] = max(worst["coast time"], float(np.max(np.abs(ct - oct_)[coast], initial=0.0)))

        def check(mask, what, cond):
            if np.any(mask & ~cond):
                failures.append((g.name, what, np.flatnonzero(mask & ~cond).tolist()))
        if precision == "f64":
            for name, row in EXACT.items():
                check(sel, name, summ[row] == osum[row])
            for name, row in ROWS.items():
                check(sel, name, relerr(summ[row], osum[row]) < (1e-7 if name == "range" else 1e-9))
        elif precision == "f64_fast":
            for name in ("steps", "rail exit time"):
                check(sel, name, summ[EXACT[name]] == osum[EXACT[name]])
            for name in ROWS:
                check(sel, name, relerr(summ[ROWS[name]], osum[ROWS[name]]) < 1e-8)
        else:
            dsteps = np.abs(summ[_abi.SUM_STEPS] - osum[_abi.SUM_STEPS])
            check(early, "steps within 25", dsteps <= 25)
            check(early & np.isin(cls, ("never_entered", "ground_step1")), "steps", dsteps == 0)
            check(early, "first apogee", relerr(summ[_abi.SUM_FIRST_APOGEE_ALT], osum[_abi.SUM_FIRST_APOGEE_ALT]) < 1e-3)
            check(coast, "coast time", np.abs(ct - oct_) <= 25 * dt + 1e-9)
            for c in LATE:   # reported, not asserted: the descent is chaotic in fp32
                m = ok & (cls == c)
                a, n = late.get(c, (0, 0))
                late[c] = (a + int(np.sum(status[m] == ostat[m])), n + int(m.sum()))
    print("%s: classes %s" % (precision, counts))
    print("%s: samples with another status word %d; worst against the oracle: %s" % (
        precision, status_diff, ", ".join("%s %.3g" % kv for kv in worst.items())))
    if late:
        print("f32: same status word as the oracle after a descent: " + ", ".join("%s %d/%d" % (c, a, n) for c, (a, n) in late.items()))
    assert not failures, failures


# ------------------------------------------------------------------ structure of the launch
@functools.lru_cache(maxsize=None)
def set_r(kind, n=200):
    pl = flatten.generate_parameter_samples(H.UNCERTAINTY, n)
    return flatten.dispersed_batch(models.Rocket(), H.make_motor(kind), models.WindModel(), H.EXAMPLE_IC, pl, H.CSV_ALT, H.CSV_WIND)


def interleaved(hb, other):
    """(the samples of `hb` spread evenly among those of `other`, the column each sample of `hb` went to)."""
    n, m = hb.n, other.n
    both = flatten.HostBatch(n + m, hb.k_wind)
    both.alt_grid = hb.alt_grid.copy()
    for name in ("ic", "rocket", "motor", "wind"):
        setattr(both, name, np.concatenate([getattr(hb, name), getattr(other, name)], axis=-1))
    key = np.concatenate([(np.arange(n) + 0.5) / n, (np.arange(m) + 0.25) / m])
    order = np.argsort(key, kind="stable")
    where = np.empty(n + m, dtype=np.int64)
    where[order] = np.arange(n + m)
    return both.take(order), where[:n]


VARIANTS = {
    # name: (set_launch, set_chunk, set_adopt, submitted, order)
    "reversed": ((64, 0, 1), -1, -1, False, "reversed"),
    "interleaved": ((64, 0, 1), -1, -1, False, "interleaved"),
    "chunk_0": ((64, 0, 1), 0, -1, False, None),
    "chunk_257": ((64, 0, 1), 257, -1, False, None),
    "chunk_4096": ((64, 0, 1), 4096, -1, False, None),        # cuts every coast-out between its latch and its end
    "adopt_0": ((64, 0, 1), 0, 0, False, None),
    "adopt_8": ((64, 0, 1), 0, 8, False, None),               # latched lanes change waves through the resume queue
    "adopt_default_submitted": ((64, 0, 1), -1, -1, True, None),
    "refill_1": ((64, 1, 1), 0, 0, False, None),              # one workgroup: finished lanes refill from the queue
    "refill_32": ((64, 1, 32), 0, 0, False, None),
    "refill_32_chunk_4096": ((256, 1, 32), 4096, 0, False, None),   # ... and from the resume queue, with latched records
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_launch_structure_does_not_change_a_bit(engine, ref, precision, variant):
    """Which lane flies a sample, with which neighbours, in how many launches, parked and resumed or handed over or not: the
    same summary and status word, bit for bit (NaN = NaN), per sample."""
    base = plain(engine, precision)
    launch, chunk, adopt, submit, order = VARIANTS[variant]
    try:
        engine.set_launch(*launch)
        engine.set_chunk(chunk)
        engine.set_adopt(adopt)
        for g in ev.groups():
            hb, where = None, np.arange(g.hb.n)
            if order == "reversed":
                where = where[::-1].copy()
                hb = g.hb.take(where)        # column j holds sample where[j]: reversing is its own inverse
            elif order == "interleaved":
                hb, where = interleaved(g.hb, set_r(g.kind))
            summ, status = fly(engine, g, precision, hb=hb, submit=submit)
            assert engine.debug_counters()[3] == 0
            assert np.array_equal(status[where], base[g.name][1]), (g.name, variant)
            assert same(summ[:, where], base[g.name][0]), (g.name, variant)
    finally:
        engine.set_launch(64, 0, 1)
        engine.set_chunk(-1)
        engine.set_adopt(-1)
    # (the coast-outs this is about are there, in this build's own results)
    ends = np.concatenate([base[g.name][1] & 0xFF for g in ev.groups()])
    assert np.sum(ends == _abi.END_COAST) >= 6


# ------------------------------------------------------------------ trajectory capture
def capture_picks():
    """{group: classes to capture there}: one sample of each class, the three altitude ranges of apogee_stop apart, the solid
    motor's coast-out (the capture instantiation reads the motor kind at run time)."""
    return {"default": ("ground_step1", "ground_unlatched", "ground_latched_chute", "altitude_unlatched"),
            "to_apogee": ("apogee_stop", "stop_flag_never_latches"), "high_chute": ("coast_120", "max_time_latched"),
            "no_time": ("never_entered",), "ascent": ("max_time_ascent",), "solid": ("coast_60",)}


@pytest.mark.parametrize("name", list(capture_picks()))
def test_capture_writes_the_oracles_records(engine, oracle, ref, name):
    """Stride 1, once with room for the whole flight and once with less (the last slot then holds the final record): the
    oracle's record counts and time stamps exactly, the states at the fp64 bars - 1e-9 of the component's largest magnitude
    in the flight for the altitude and the vertical speed up to the first apogee (what the summary's 1e-9 rows are made of),
    1e-7 for every component over the whole flight (the bar of the range, which the descent's error growth sets)."""
    g = next(x for x in ev.groups() if x.name == name)
    osum, ostat, cls, ok = ref[name]
    ids = []
    for c in capture_picks()[name]:
        m = ok & (cls == c)
        if c == "apogee_stop":
            ids += [int(np.flatnonzero(m & (ev.tier(osum) == t))[0]) for t in (300, 120, 60)]
        else:
            ids.append(int(np.flatnonzero(m)[0]))
    steps = osum[_abi.SUM_STEPS].astype(np.int64)
    long_ids = [i for i in ids if steps[i] > 1]
    runs = [(ids, int(steps[ids].max()) + 2)]                        # room for every record
    if long_ids:                                                     # half of the shortest real flight: every one is cut
        runs.append((long_ids, (int(steps[long_ids].min()) + 1) // 2))
    if len(long_ids) < len(ids):                                     # a flight of one step or none: a single slot
        runs.append((ids, 1))
    cfg = ev.config(name)
    for ids, cap in runs:
        summ, status, traj, tlen = fly(engine, g, "f64", traj_ids=ids, traj_stride=1, traj_cap=cap)
        _, _, otraj, otlen = oracle.run_batch(cfg, g.hb, flags=g.flags, traj_ids=ids, traj_stride=1, traj_cap=cap)
        assert np.array_equal(tlen, otlen), (name, cap, tlen, otlen)
        for m, i in enumerate(ids):
            k = int(otlen[m])
            assert k == min(cap, int(osum[_abi.SUM_STEPS, i]) + 1)
            assert traj[m, 0, 0] == otraj[m, 0, 0] and traj[m, k - 1, 0] == otraj[m, k - 1, 0], (name, cap, i)
            assert np.array_equal(traj[m, :k, 0], otraj[m, :k, 0]), (name, cap, i)
            scale = np.maximum(np.max(np.abs(otraj[m, :k, 1:]), axis=0), 1e-12)
            err = np.abs(traj[m, :k, 1:] - otraj[m, :k, 1:]) / scale
            up = otraj[m, :k, 0] - osum[_abi.SUM_RAIL_EXIT_TIME, i] <= osum[_abi.SUM_FIRST_APOGEE_TIME, i]
            print("%s cap %d sample %d (%s): %d records, worst state error %.3g, to the first apogee z %.3g vz %.3g" % (
                name, cap, i, cls[i], k, err.max(), err[up, 2].max(initial=0.0), err[up, 5].max(initial=0.0)))
            assert err.max() < 1e-7, (name, cap, i)
            assert err[up, 2].max(initial=0.0) < 1e-9 and err[up, 5].max(initial=0.0) < 1e-9, (name, cap, i)
        assert np.array_equal(status[ok], ostat[ok]) and same(summ, plain(engine, "f64")[name][0])   # capturing changes no summary
    if name == "no_time":
        # a capture of ONE record is a valid input of what reads captures: the diagnostic histories of that record against
        # the oracle's, at the 1e-9 of test_extract_histories_vs_oracle (entries that are zero up to rounding are held to
        # 1e-9 of the record's largest entry: a single record has no history to take a column's scale from)
        from erpl_monte_carlo_sim_amd.engine import DeviceBatch
        i = ids[0]
        assert int(tlen[0]) == 1
        t_rail = float(osum[_abi.SUM_RAIL_EXIT_TIME, i])
        db = DeviceBatch.from_host(g.hb, engine.device, _abi.PREC_F64)
        got = engine.extract_histories(db, i, torch.as_tensor(traj[0, :1], device=engine.device), t_rail).cpu().numpy()
        exp = oracle.extract(cfg, g.hb.take([i]), traj[0, :1], t_rail)
        assert got.shape == exp.shape == (1, _abi.DIAG_DIM) and np.array_equal(np.isfinite(got), np.isfinite(exp))
        fin = np.isfinite(exp)
        scale = np.maximum(np.abs(exp), 1e-9 * np.max(np.abs(exp[fin])))
        assert np.max((np.abs(got - exp) / scale)[fin]) < 1e-9
