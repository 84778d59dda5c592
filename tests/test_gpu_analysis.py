"""erpl_mc_analyze on the device (outlier filter, moments, exact radix selection) against NumPy on host copies of the
same tensors: analysis.outlier_mask / outlier_reasons for validity and reason bits, np.sort of the masked finite values
for the order statistics, np.mean / np.std / np.quantile (np.percentile with the fraction taken as it is, not through
100 * q / 100) for the rest.

Exact, no tolerance: n_valid, n_outliers, reason counts, termination counts, n_status_nan, per-row count / min / max,
every order_lo / order_hi, every reason byte.  Rounded quantities (the bar of device_statistics against
tests/golden/stats.json, scaled because several rows are centred on zero):
    |mean - np.mean| <= 1e-12 * mean(|x|),  |std - np.std| <= 1e-12 * np.std,
    |quantile - np.quantile| <= 1e-12 * max(|order_lo|, |order_hi|)."""
import ctypes as C

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models, sampling

import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-12
DEFAULT_ROWS = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
DEFAULT_Q = [0.05, 0.25, 0.5, 0.75, 0.95]
ALL_Q = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 1.0 / 3.0]


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


def bits_of(strings):
    """Reason bits rebuilt from the strings of analysis.outlier_reasons."""
    b = 0
    for s in strings:
        if s == "non-finite values":
            b |= _abi.WHY_NON_FINITE
        elif s == "apogee exceeds theoretical energy limit":
            b |= _abi.WHY_ENERGY
        elif s.startswith("apogee") and " km > " in s:
            b |= _abi.WHY_APOGEE_HIGH
        elif s.startswith("apogee") and " m < " in s:
            b |= _abi.WHY_APOGEE_LOW
        elif s.startswith("range"):
            b |= _abi.WHY_RANGE
        elif s.startswith("flight time"):
            b |= _abi.WHY_FLIGHT_TIME
        else:
            raise AssertionError(s)
    return b


def host_bits(summ):
    apo, rng, ft = summ[_abi.SUM_APOGEE_ALT], summ[_abi.SUM_RANGE], summ[_abi.SUM_FLIGHT_TIME]
    with np.errstate(invalid="ignore"):
        return np.array([bits_of(analysis.outlier_reasons(a, r, f)) for a, r, f in zip(apo, rng, ft)], dtype=np.uint8)


def check_against_numpy(res, why, summ, status, rows, qs, skip_std=()):
    """res: _abi.ErplAnalysis, why: uint8 tensor; summ / status: the host copies the device tensors were made from."""
    n = summ.shape[1]
    bad = analysis.outlier_mask(summ[_abi.SUM_APOGEE_ALT], summ[_abi.SUM_RANGE], summ[_abi.SUM_FLIGHT_TIME])
    bits = host_bits(summ)
    assert np.array_equal(bits != 0, bad)                       # the two pinned host functions agree with each other
    assert np.array_equal(why.cpu().numpy(), bits)              # every sample's reason byte
    assert res.n == n and res.n_valid == int((~bad).sum()) and res.n_outliers == int(bad.sum())
    assert list(res.reason_counts) == [int(((bits >> k) & 1).sum()) for k in range(6)]
    if status is None:
        assert list(res.termination_counts) == [0] * 5 and res.n_status_nan == 0 and res.n_incomplete == 0
    else:
        assert list(res.termination_counts) == [int(((status & 0xFF) == k).sum()) for k in range(5)]
        assert res.n_status_nan == int(((status & _abi.ST_NAN) != 0).sum())
        assert res.n_incomplete == int(((status & _abi.ST_INCOMPLETE) != 0).sum())
    for j, r in enumerate(rows):
        got = res.row[j]
        x = summ[r][~bad & np.isfinite(summ[r])]
        assert got.count == len(x), r
        if len(x) == 0:
            vals = [got.mean, got.std, got.min, got.max] + list(got.quantile) + list(got.order_lo) + list(got.order_hi)
            assert all(np.isnan(v) for v in vals), r
            continue
        xs = np.sort(x)
        assert got.min == xs[0] and got.max == xs[-1], r
        mean, std = np.mean(x), np.std(x)
        print(f"row {r}: count {len(x)}, mean err {abs(got.mean - mean) / max(np.mean(np.abs(x)), 1e-300):.2e} of mean|x|, "
              f"std err {abs(got.std - std) / std if std > 0 else abs(got.std - std):.2e}")
        assert abs(got.mean - mean) <= TOL * np.mean(np.abs(x)), (r, got.mean, mean)
        if r not in skip_std:
            assert abs(got.std - std) <= TOL * std, (r, got.std, std)
        for k, q in enumerate(qs):
            pos = q * (len(x) - 1)
            lo = int(np.floor(pos))
            hi = min(lo + 1, len(x) - 1)
            assert got.order_lo[k] == xs[lo] and got.order_hi[k] == xs[hi], (r, q, got.order_lo[k], xs[lo], got.order_hi[k], xs[hi])
            ref = np.quantile(x, q)
            assert abs(got.quantile[k] - ref) <= TOL * max(abs(xs[lo]), abs(xs[hi])), (r, q, got.quantile[k], ref)
        for k in range(len(qs), _abi.ANALYSIS_MAX_Q):
            assert np.isnan(got.quantile[k])


def run(engine, summ, status, rows=None, qs=None):
    ds = torch.from_numpy(np.ascontiguousarray(summ)).to(engine.device)
    dt = None if status is None else torch.from_numpy(status).to(engine.device)
    res, why = engine.analyze(ds, dt, rows=rows, quantiles=qs, reasons=True)
    return res, why, ds, dt


# ------------------------------------------------------------------ 1: the reference's own numbers
def test_golden_statistics_of_the_reference(engine):
    g = H.load_json("stats.json")
    inp = g["inputs"]
    keep = [i for i in range(len(inp["apogee_altitude"])) if i != inp["none_index"]]
    summ = np.zeros((16, len(keep)))
    summ[_abi.SUM_APOGEE_ALT] = [inp["apogee_altitude"][i] for i in keep]
    summ[_abi.SUM_RANGE] = [inp["range"][i] for i in keep]
    summ[_abi.SUM_FLIGHT_TIME] = [inp["flight_time"][i] for i in keep]
    status = np.zeros(len(keep), dtype=np.int32)
    res, why, ds, dt = run(engine, summ, status)
    check_against_numpy(res, why, summ, status, DEFAULT_ROWS, DEFAULT_Q)
    assert res.n_valid == g["n_samples"] and res.n_outliers == g["n_outliers"]
    out = analysis.native_statistics(ds, dt, engine=engine)
    assert out["n_samples"] == g["n_samples"] and out["n_outliers"] == g["n_outliers"] and out["n_failed"] == 0
    for key in ("apogee_altitude", "range", "flight_time"):
        ref = g[key]
        assert out[key]["min"] == ref["min"] and out[key]["max"] == ref["max"]
        assert abs(out[key]["mean"] - ref["mean"]) <= TOL * abs(ref["mean"]), key
        assert abs(out[key]["std"] - ref["std"]) <= TOL * ref["std"], key
        for a, b in zip(out[key]["percentiles"], ref["percentiles"]):
            assert abs(a - b) <= TOL * abs(b), key


# ------------------------------------------------------------------ 2: values on and just past the bounds
def test_bounds_nan_and_inf(engine):
    rng = np.random.RandomState(11)
    n = 5000
    summ = np.zeros((16, n))
    summ[_abi.SUM_APOGEE_ALT] = rng.normal(25000, 20000, n)
    summ[_abi.SUM_RANGE] = np.abs(rng.normal(50000, 90000, n))
    summ[_abi.SUM_FLIGHT_TIME] = rng.normal(300, 150, n)
    summ[_abi.SUM_APOGEE_ALT, :7] = [np.nan, np.inf, 50.0, 100.0, 80000.0, 88073.4, -np.inf]
    summ[_abi.SUM_RANGE, 7:10] = [np.nan, 200000.0, 200000.1]
    status = rng.randint(0, 4, n).astype(np.int32)
    res, why, ds, dt = run(engine, summ, status)
    check_against_numpy(res, why, summ, status, DEFAULT_ROWS, DEFAULT_Q)
    w = why.cpu().numpy()
    apo_bits = _abi.WHY_NON_FINITE | _abi.WHY_APOGEE_HIGH | _abi.WHY_APOGEE_LOW | _abi.WHY_ENERGY
    assert list(w[:7] & apo_bits) == [1, 1 | 2 | 32, 4, 0, 0, 2 | 32, 1 | 4]      # on a bound is inside it
    assert list(w[7:10] & (_abi.WHY_NON_FINITE | _abi.WHY_RANGE)) == [1, 0, 8]
    # the torch path on the same tensors
    ref, got = analysis.device_statistics(ds, dt), analysis.native_statistics(ds, dt, engine=engine)
    assert got["n_samples"] == ref["n_samples"] and got["n_outliers"] == ref["n_outliers"]
    assert got["termination_counts"] == ref["termination_counts"] and got["n_non_finite"] == ref["n_non_finite"]
    assert torch.equal(got["valid_mask"], ref["valid_mask"])
    assert sum(got["reason_counts"].values()) >= got["n_outliers"] > 0


# ------------------------------------------------------------------ 3: a million samples, every row, awkward values
def big_case():
    rng = np.random.RandomState(2024)
    n = 2 ** 20 + 12345
    s = np.zeros((16, n))

    def sprinkle(x, frac=0.30):
        k = rng.random_sample(n) < frac
        x[k] = rng.choice([np.nan, np.inf, -np.inf], size=int(k.sum()))
        return x

    s[0] = rng.normal(25000, 20000, n)                       # apogee
    s[1] = rng.normal(0, 3000, n)                            # negative keys
    s[2] = rng.randint(2000, 60001, n).astype(np.float64)    # integers as doubles
    s[3] = 7.0                                               # a constant: every lane of every wave in one bin
    s[4] = sprinkle(np.abs(rng.normal(50000, 90000, n)))     # range, 30 % NaN / +-inf
    s[5] = np.round(rng.normal(300, 150, n) / 2) * 2         # flight time: a few hundred distinct values
    s[6] = sprinkle(rng.normal(1000, 10, n))                 # non-finite values in a row that is not a filter row
    z = rng.choice([0.0, -0.0, 1e-300, -1e-300, 3e-300, -2.5e-300], size=n)
    s[7] = z * np.where(np.abs(z) > 0, rng.uniform(0.5, 2.0, n), 1.0)   # +-0.0 among values around 1e-300
    s[8] = rng.normal(0, 3000, n)
    s[9] = rng.uniform(-1.0, 1.0, n)
    s[10] = rng.exponential(1.0, n)
    s[11] = rng.normal(-5000, 100, n)                        # negative throughout
    s[12] = rng.normal(0, 1, n) * 1e90
    s[13] = rng.lognormal(0, 3, n)
    s[14] = np.round(rng.normal(0, 2, n))                    # a dozen distinct values around zero, -0.0 among them
    s[15] = rng.normal(1e-5, 1e-7, n)
    status = rng.randint(0, 5, n).astype(np.int32)
    status |= (rng.random_sample(n) < 0.3).astype(np.int32) * _abi.ST_NAN
    status |= (rng.random_sample(n) < 0.5).astype(np.int32) * _abi.ST_CHUTE
    return s, status


def test_a_million_samples_all_rows_exact_and_repeatable(engine):
    summ, status = big_case()
    n = summ.shape[1]
    rows = list(range(16))
    res, why, ds, dt = run(engine, summ, status, rows, ALL_Q)
    assert n // 4 < res.n_valid < 3 * n // 4
    check_against_numpy(res, why, summ, status, rows, ALL_Q, skip_std=(7,))   # squares of 1e-300 underflow
    for j in rows:          # q = 0 and q = 1 are min and max
        assert res.row[j].quantile[0] == res.row[j].min == res.row[j].order_lo[0]
        assert res.row[j].quantile[6] == res.row[j].max == res.row[j].order_hi[6]
    # repeatability: the same inputs into zero-initialised result blocks give the same bytes
    spec = engine.analysis_defaults()
    spec.n_rows, spec.n_q = 16, len(ALL_Q)
    spec.rows[:16] = rows
    spec.q[:len(ALL_Q)] = ALL_Q
    blocks = []
    for _ in range(2):
        r = _abi.ErplAnalysis()
        C.memset(C.byref(r), 0, C.sizeof(r))
        rc = engine.lib.erpl_mc_analyze(engine._ctx, C.c_void_p(ds.data_ptr()), C.c_void_p(dt.data_ptr()), n, C.byref(spec),
                                        C.byref(r), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        blocks.append(bytes(r))
    assert blocks[0] == blocks[1] == bytes(res)


# ------------------------------------------------------------------ 4: tiny batches, nothing valid
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_tiny_batches(engine, n):
    rng = np.random.RandomState(n)
    summ = rng.normal(0, 100, (16, n))
    summ[_abi.SUM_APOGEE_ALT] = rng.uniform(200, 70000, n)
    summ[_abi.SUM_RANGE] = rng.uniform(0, 150000, n)
    summ[_abi.SUM_FLIGHT_TIME] = rng.uniform(10, 500, n)
    if n > 2:
        summ[_abi.SUM_APOGEE_ALT, 1] = 90000.0
        summ[_abi.SUM_IMPACT_X, 2] = np.nan
    status = rng.randint(0, 5, n).astype(np.int32)
    rows = [_abi.SUM_APOGEE_ALT, _abi.SUM_IMPACT_X, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, _abi.SUM_MAX_SPEED]
    res, why, ds, dt = run(engine, summ, status, rows, ALL_Q)
    check_against_numpy(res, why, summ, status, rows, ALL_Q)
    res, why, _, _ = run(engine, summ, None)
    check_against_numpy(res, why, summ, None, DEFAULT_ROWS, DEFAULT_Q)


def test_nothing_valid_is_no_error_of_the_c_call(engine):
    summ = np.full((16, 100), 1.0)
    summ[_abi.SUM_APOGEE_ALT, :50] = np.nan
    summ[_abi.SUM_APOGEE_ALT, 50:] = 1e6
    res, why, ds, _ = run(engine, summ, None)
    assert res.n_valid == 0 and res.n_outliers == 100
    check_against_numpy(res, why, summ, None, DEFAULT_ROWS, DEFAULT_Q)
    for j in range(3):
        assert res.row[j].count == 0 and np.isnan(res.row[j].mean) and np.isnan(res.row[j].order_lo[0])
    with pytest.raises(ValueError, match="No physically reasonable simulation results after outlier filtering"):
        analysis.native_statistics(ds, engine=engine)


# ------------------------------------------------------------------ 5: a real run
def test_real_run_agrees_with_the_torch_path(engine):
    db = sampling.synthetic_dispersions(24000, models.Rocket(), H.make_motor("liquid"), models.WindModel(), H.EXAMPLE_IC,
                                        engine.device, precision=_abi.PREC_F64_FAST, seed=4242, engine=engine)
    summ, status = engine.run(db)
    torch.cuda.synchronize()
    ref = analysis.device_statistics(summ, status)
    got = analysis.native_statistics(summ, status)            # the shared engine of the tensors' device
    res, why = engine.analyze(summ, status, reasons=True)
    check_against_numpy(res, why, summ.cpu().numpy(), status.cpu().numpy(), DEFAULT_ROWS, DEFAULT_Q)
    assert got["n_samples"] == ref["n_samples"] and got["n_outliers"] == ref["n_outliers"] and got["n_failed"] == 0
    assert got["termination_counts"] == ref["termination_counts"] and got["n_non_finite"] == ref["n_non_finite"]
    assert torch.equal(got["valid_mask"], ref["valid_mask"])
    assert torch.equal(got["outlier_reason_bits"], why)
    print("valid", got["n_samples"], "of 24000;", got["reason_counts"])
    for j, key in enumerate(("apogee_altitude", "range", "flight_time")):
        x = summ[DEFAULT_ROWS[j]][ref["valid_mask"]].cpu().numpy()
        assert got[key]["min"] == ref[key]["min"] and got[key]["max"] == ref[key]["max"]
        assert abs(got[key]["mean"] - ref[key]["mean"]) <= TOL * np.mean(np.abs(x)), key
        assert abs(got[key]["std"] - ref[key]["std"]) <= TOL * ref[key]["std"], key
        rows = got["rows"][DEFAULT_ROWS[j]]
        for a, b, lo, hi in zip(got[key]["percentiles"], ref[key]["percentiles"], rows["order_lo"], rows["order_hi"]):
            assert abs(a - b) <= TOL * max(abs(lo), abs(hi)), key


# ------------------------------------------------------------------ 6: samples that were never integrated
def test_incomplete_samples_are_reported(engine):
    rng = np.random.RandomState(6)
    n = 1000
    summ = np.zeros((16, n))
    summ[_abi.SUM_APOGEE_ALT] = rng.uniform(200, 70000, n)
    summ[_abi.SUM_RANGE] = rng.uniform(0, 150000, n)
    summ[_abi.SUM_FLIGHT_TIME] = rng.uniform(10, 500, n)
    status = rng.randint(0, 4, n).astype(np.int32)
    status[[5, 500, 999]] = _abi.ST_INCOMPLETE
    ds, dt = torch.from_numpy(summ).to(engine.device), torch.from_numpy(status).to(engine.device)
    spec, res = engine.analysis_defaults(), _abi.ErplAnalysis()
    rc = engine.lib.erpl_mc_analyze(engine._ctx, C.c_void_p(ds.data_ptr()), C.c_void_p(dt.data_ptr()), n, C.byref(spec),
                                    C.byref(res), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _abi.ERR_INCOMPLETE and res.n_incomplete == 3 and b"ERPL_ST_INCOMPLETE" in engine.lib.erpl_mc_last_error()
    assert res.n == n and res.n_valid == n and res.row[0].count == n      # the result is filled all the same
    with pytest.raises(_abi.IncompleteBatch):
        engine.analyze(ds, dt)
    with pytest.raises(_abi.IncompleteBatch):
        analysis.native_statistics(ds, dt, engine=engine)


# ------------------------------------------------------------------ stream order
def test_analysis_is_ordered_behind_the_stream(engine):
    """The summary is produced on a side stream; the current stream waits for it on the device and the analysis is
    enqueued there with no host synchronisation in between.  A dependency check, run once."""
    rng = np.random.RandomState(3)
    n = 1 << 18
    base = np.zeros((16, n))
    base[_abi.SUM_APOGEE_ALT] = rng.normal(25000, 20000, n)
    base[_abi.SUM_RANGE] = np.abs(rng.normal(50000, 90000, n))
    base[_abi.SUM_FLIGHT_TIME] = rng.normal(300, 150, n)
    src = torch.from_numpy(base).to(engine.device)
    ds = torch.full((16, n), float("nan"), dtype=torch.float64, device=engine.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=engine.device)
    with torch.cuda.stream(side):
        tmp = src
        for _ in range(40):          # some work in front of the copy, all on the side stream
            tmp = tmp * 1.0
        ds.copy_(tmp)
    torch.cuda.current_stream(engine.device).wait_stream(side)
    res, why = engine.analyze(ds, reasons=True)
    check_against_numpy(res, why, base, None, DEFAULT_ROWS, DEFAULT_Q)


# ------------------------------------------------------------------ the Python layer
def test_python_layer_refuses_what_the_kernels_cannot_take(engine):
    ok = torch.zeros((16, 8), dtype=torch.float64, device=engine.device)
    for bad in (ok.cpu(), ok.float(), ok[:, ::2], ok[:15], ok.t().contiguous()):
        with pytest.raises(ValueError):
            engine.analyze(bad)
    with pytest.raises(ValueError):
        engine.analyze(ok, torch.zeros(8, dtype=torch.int64, device=engine.device))
    with pytest.raises(ValueError):
        engine.analyze(ok, torch.zeros(9, dtype=torch.int32, device=engine.device))
    with pytest.raises(_abi.ErplError, match="twice"):
        engine.analyze(ok, rows=[1, 1])
    out = analysis.native_statistics(ok + 500.0, rows=[_abi.SUM_IMPACT_Y], quantiles=[0.5], engine=engine)
    assert list(out["rows"]) == [_abi.SUM_IMPACT_Y] and out["rows"][_abi.SUM_IMPACT_Y]["percentiles"] == [500.0]
    assert out["apogee_altitude"]["mean"] == 500.0 and out["apogee_altitude"]["std"] == 0.0 and "termination_counts" not in out


# ------------------------------------------------------------------ 10: the reason bytes grow with n and never shrink
def test_workspace_regrow_gives_the_bytes_of_a_fresh_engine(engine):
    """257 and 4099 samples are 2 and 17 workgroups of ERPL_ANA_BLOCK, one sample past a block boundary: the second call
    replaces the first one's reason bytes, the third runs in the larger buffer.  The library promises repeatable bytes, so
    each result equals, bit for bit, what a fresh engine gives for that call alone."""
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    for n in (257, 4099, 257):
        summ, status = H.synthetic_summary(n, 40 + n)
        res, why, ds, dt = run(engine, summ, status)
        assert 0 < res.n_valid < n
        fresh = TrajectoryEngine(engine.device)
        ref, ref_why = fresh.analyze(ds, dt, reasons=True)
        fresh.close()
        assert bytes(res) == bytes(ref) and torch.equal(why, ref_why), n
