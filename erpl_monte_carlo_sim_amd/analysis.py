"""Outlier filter + statistics of the Monte Carlo driver (thin host glue).

Same bounds, keys and reason strings as monte_carlo.py:337-398 / :400-473 of the reference, but
evaluated on arrays (one pass over the gathered per-sample summaries) instead of a Python loop
over result dicts.  Checked against tests/golden/stats.json.
"""
import math

import numpy as np

MAX_REASONABLE_APOGEE = 80000.0
MAX_REASONABLE_RANGE = 200000.0
MAX_REASONABLE_FLIGHT_TIME = 600.0
MIN_REASONABLE_APOGEE = 100.0
_THEORETICAL_MAX_ALTITUDE = 1200.0 ** 2 / (2 * 9.81)


def outlier_reasons(apogee, range_val, flight_time):
    """Reason strings of one sample, in the reference's order (monte_carlo.py:356-388)."""
    reasons = []
    if not np.isfinite(apogee) or not np.isfinite(range_val) or not np.isfinite(flight_time):
        reasons.append("non-finite values")
    if apogee > MAX_REASONABLE_APOGEE:
        reasons.append(f"apogee {apogee/1000:.1f} km > {MAX_REASONABLE_APOGEE/1000:.1f} km")
    elif apogee < MIN_REASONABLE_APOGEE:
        reasons.append(f"apogee {apogee:.1f} m < {MIN_REASONABLE_APOGEE:.1f} m")
    if range_val > MAX_REASONABLE_RANGE:
        reasons.append(f"range {range_val/1000:.1f} km > {MAX_REASONABLE_RANGE/1000:.1f} km")
    if flight_time > MAX_REASONABLE_FLIGHT_TIME:
        reasons.append(f"flight time {flight_time:.1f} s > {MAX_REASONABLE_FLIGHT_TIME:.1f} s")
    if apogee > _THEORETICAL_MAX_ALTITUDE * 1.2:
        reasons.append("apogee exceeds theoretical energy limit")
    return reasons


def outlier_mask(apogee, range_val, flight_time):
    """Vectorised form of the same tests: True where the sample is an outlier."""
    apogee, range_val, flight_time = (np.asarray(a, dtype=np.float64) for a in (apogee, range_val, flight_time))
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(apogee) | ~np.isfinite(range_val) | ~np.isfinite(flight_time)
        bad |= (apogee > MAX_REASONABLE_APOGEE) | (apogee < MIN_REASONABLE_APOGEE)
        bad |= range_val > MAX_REASONABLE_RANGE
        bad |= flight_time > MAX_REASONABLE_FLIGHT_TIME
        bad |= apogee > _THEORETICAL_MAX_ALTITUDE * 1.2
    return bad


def calc_stats(values):
    """monte_carlo.py:444-459."""
    values = np.asarray(values, dtype=np.float64)
    values = values[np.isfinite(values)]
    if len(values) == 0:
        nan = float("nan")
        return {"mean": nan, "std": nan, "min": nan, "max": nan, "percentiles": [nan] * 5}
    return {"mean": float(np.mean(values)), "std": float(np.std(values)), "min": float(np.min(values)),
            "max": float(np.max(values)), "percentiles": np.percentile(values, [5, 25, 50, 75, 95]).tolist()}


def parameter_ranges(param_dicts):
    """Observed min/max of every sampled parameter over the valid samples (monte_carlo.py:425-441)."""
    out = {}
    for params in param_dicts:
        for key, val in params.items():
            arr = np.array(val)
            if key not in out:
                out[key] = {"min": arr.astype(float), "max": arr.astype(float)}
            else:
                out[key]["min"] = np.minimum(out[key]["min"], arr)
                out[key]["max"] = np.maximum(out[key]["max"], arr)
    for key in out:
        out[key]["min"] = out[key]["min"].tolist()
        out[key]["max"] = out[key]["max"].tolist()
    return out


def analyze(results, verbose=False):
    """`MonteCarloAnalyzer._analyze_results` on a list of per-sample dicts (None = failed sample).
    Raises the reference's ValueErrors when nothing (reasonable) is left (monte_carlo.py:405-412)."""
    initial = [r for r in results if r is not None]
    if len(initial) == 0:
        raise ValueError("No valid simulation results")
    apo = np.array([r.get("apogee_altitude", 0) for r in initial], dtype=np.float64)
    rng = np.array([r.get("range", 0) for r in initial], dtype=np.float64)
    ft = np.array([r.get("flight_time", 0) for r in initial], dtype=np.float64)
    bad = outlier_mask(apo, rng, ft)
    valid, outliers = [], []
    for r, b, a_, r_, f_ in zip(initial, bad, apo, rng, ft):
        if b:
            r["outlier_reasons"] = outlier_reasons(a_, r_, f_)
            outliers.append(r)
            if verbose:
                print(f"Filtered outlier simulation {r.get('simulation_id', '?')}: {', '.join(r['outlier_reasons'])}")
        else:
            valid.append(r)
    if verbose:
        print(f"Physics-based filtering: {len(valid)} valid, {len(outliers)} outliers")
    if len(valid) == 0:
        raise ValueError("No physically reasonable simulation results after outlier filtering")
    ok = ~bad
    return {
        "n_samples": len(valid),
        "n_failed": len(results) - len(initial),
        "n_outliers": len(outliers),
        "apogee_altitude": calc_stats(apo[ok]),
        "range": calc_stats(rng[ok]),
        "flight_time": calc_stats(ft[ok]),
        "results": valid,
        "outliers": outliers,
        "parameter_ranges_observed": parameter_ranges(r.get("parameters", {}) for r in valid),
    }


def device_statistics(summary, status=None):
    """Outlier filter + statistics on the gathered [16, n] summary tensor WITHOUT leaving the device
    (SURVEY.md §8f-3): the same bounds as `outlier_mask` and the same statistics as `calc_stats`
    (NumPy-style linear-interpolated percentiles, population std) with torch ops, for the 100 k - 10 M
    sample runs where a Python list of result dicts is not an option.  Works on CPU tensors too."""
    import torch
    from . import _abi
    s = summary.to(torch.float64)
    apo, rng, ft = s[_abi.SUM_APOGEE_ALT], s[_abi.SUM_RANGE], s[_abi.SUM_FLIGHT_TIME]
    bad = ~torch.isfinite(apo) | ~torch.isfinite(rng) | ~torch.isfinite(ft)
    bad |= (apo > MAX_REASONABLE_APOGEE) | (apo < MIN_REASONABLE_APOGEE)
    bad |= rng > MAX_REASONABLE_RANGE
    bad |= ft > MAX_REASONABLE_FLIGHT_TIME
    bad |= apo > _THEORETICAL_MAX_ALTITUDE * 1.2
    ok = ~bad
    n_valid = int(ok.sum().item())
    if n_valid == 0:
        raise ValueError("No physically reasonable simulation results after outlier filtering")
    q = torch.tensor([0.05, 0.25, 0.5, 0.75, 0.95], dtype=torch.float64, device=s.device)

    def stats(v):
        v = v[ok]
        # torch.quantile is limited to 16 M elements; sort-based linear interpolation has no limit
        vs, _ = torch.sort(v)
        pos = q * (vs.numel() - 1)
        lo = pos.floor().long()
        hi = torch.clamp(lo + 1, max=vs.numel() - 1)
        frac = pos - lo.to(torch.float64)
        pct = vs[lo] + (vs[hi] - vs[lo]) * frac
        return {"mean": float(v.mean().item()), "std": float(v.std(unbiased=False).item()),
                "min": float(vs[0].item()), "max": float(vs[-1].item()), "percentiles": pct.tolist()}

    out = {"n_samples": n_valid, "n_failed": 0, "n_outliers": int(bad.sum().item()),
           "apogee_altitude": stats(apo), "range": stats(rng), "flight_time": stats(ft),
           "valid_mask": ok}
    if status is not None:
        st = status.to(torch.int64) & 0xFF
        out["termination_counts"] = {name: int((st == code).sum().item()) for code, name in
                                     enumerate(("max_time", "ground_impact", "excessive_altitude",
                                                "coast_timeout", "apogee"))}
        out["n_non_finite"] = int(((status.to(torch.int64) & _abi.ST_NAN) != 0).sum().item())
        n_inc = int(((status.to(torch.int64) & _abi.ST_INCOMPLETE) != 0).sum().item())
        if n_inc:   # a lane hand-over timed out: these samples were never integrated (include/erpl_mc.h)
            raise _abi.IncompleteBatch(f"{n_inc} sample(s) carry ERPL_ST_INCOMPLETE: refusing to compute statistics on them")
    return out


def _engine_of(summary, engine):
    if engine is None:
        from .simulator import shared_engine
        engine = shared_engine(summary.device)
    return engine


def _filter(summary, status, engine):
    """First step of every function that works on the filtered population: (engine, erpl_mc_analyze result without row
    statistics, reason bytes [n] uint8 on the device - the mask of the call that follows)."""
    engine = _engine_of(summary, engine)
    res, why = engine.analyze(summary, status, rows=[], quantiles=[], reasons=True)
    return engine, res, why


def _row_dict(r, n_q):
    return {"count": int(r.count), "mean": r.mean, "std": r.std, "min": r.min, "max": r.max,
            "percentiles": list(r.quantile[:n_q]), "order_lo": list(r.order_lo[:n_q]), "order_hi": list(r.order_hi[:n_q])}


def native_statistics(summary, status=None, engine=None, rows=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95)):
    """`device_statistics` through the library's own kernels (erpl_mc_analyze) instead of torch ops: the same keys with
    the same meaning, from a handful of streaming passes and an exact radix selection instead of three full sorts, plus
    `reason_counts` (why samples were filtered), `outlier_reason_bits` (uint8 device tensor, _abi.WHY_*) and `rows`
    (statistics of every requested summary row, with the two order statistics behind each percentile).
    CUDA tensors only: `device_statistics` stays the implementation for CPU tensors."""
    from . import _abi
    engine = _engine_of(summary, engine)
    named = (("apogee_altitude", _abi.SUM_APOGEE_ALT), ("range", _abi.SUM_RANGE), ("flight_time", _abi.SUM_FLIGHT_TIME))
    wanted = [r for _, r in named] if rows is None else [int(r) for r in rows]
    described = wanted + [r for _, r in named if r not in wanted]
    quantiles = [float(q) for q in quantiles]
    try:
        res, why = engine.analyze(summary, status, rows=described, quantiles=quantiles, reasons=True)
    except _abi.IncompleteBatch as e:
        raise _abi.IncompleteBatch(f"{e}: refusing to compute statistics on them") from None
    if res.n_valid == 0:
        raise ValueError("No physically reasonable simulation results after outlier filtering")
    stats = {r: _row_dict(res.row[j], len(quantiles)) for j, r in enumerate(described)}
    out = {"n_samples": int(res.n_valid), "n_failed": 0, "n_outliers": int(res.n_outliers)}
    for name, r in named:
        out[name] = {k: stats[r][k] for k in ("mean", "std", "min", "max", "percentiles")}
    out["valid_mask"] = why == 0
    out["reason_counts"] = {name: int(res.reason_counts[k]) for k, name in enumerate(_abi.WHY_NAMES)}
    out["outlier_reason_bits"] = why
    out["rows"] = {r: stats[r] for r in wanted}
    if status is not None:
        out["termination_counts"] = {name: int(res.termination_counts[k]) for k, name in enumerate(_abi.END_NAMES)}
        out["n_non_finite"] = int(res.n_status_nan)
    return out


def native_distributions(summary, status=None, engine=None, bins=50, rows=None):
    """The histograms `plot_results` draws (monte_carlo.py:568-592), counted on the device: erpl_mc_analyze for the reason
    bytes, then erpl_mc_histogram over the samples that carry none - the filtered population `analysis['results']` holds.
    rows: summary rows (default apogee, range, flight time); bins: one int or one per row.  Returns {row: {'edges',
    'counts', 'counted'}} with NumPy arrays equal to np.histogram(valid finite values of the row, bins), plus
    'valid_mask' (bool device tensor), 'outlier_reason_bits', 'n_samples' and 'n_outliers'."""
    from . import _abi
    rows = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME] if rows is None else [int(r) for r in rows]
    engine, res, why = _filter(summary, status, engine)
    edges, counts, info = engine.histogram(summary, why, rows=rows, bins=bins)
    out = {r: {"edges": edges[j], "counts": counts[j], "counted": int(info["counted"][j])} for j, r in enumerate(rows)}
    out["valid_mask"] = why == 0
    out["outlier_reason_bits"] = why
    out["n_samples"], out["n_outliers"] = int(res.n_valid), int(res.n_outliers)
    return out


def landing_dispersion(summary, status=None, engine=None, target=None, levels=(0.5, 0.9, 0.99),
                       quantiles=(0.5, 0.9, 0.95, 0.99)):
    """Where the filtered population comes down (erpl_mc_analyze for the reason bytes, then erpl_mc_dispersion on the
    impact point): mean, covariance, confidence ellipses with their empirical content and the miss distance about
    `target` ((x, y), default the launch site at the origin) with its exact quantiles; 'cep' is the median miss distance.
    The dict of TrajectoryEngine.dispersion plus 'n_samples' / 'n_outliers' of the filter."""
    engine, res, why = _filter(summary, status, engine)
    out = engine.dispersion(summary, why, centre=(0.0, 0.0) if target is None else target, levels=levels,
                            quantiles=quantiles)
    out["n_samples"], out["n_outliers"] = int(res.n_valid), int(res.n_outliers)
    return out


def wilson_interval(k, n, level=0.95):
    """The Wilson score interval (lo, hi) of a proportion k / n at confidence `level` (Wilson 1927): with p = k / n and z
    the standard normal quantile of 1 - (1 - level) / 2, (p + z^2 / 2n -+ z sqrt(p (1 - p) / n + z^2 / 4n^2)) / (1 + z^2 / n),
    clipped to [0, 1].  n == 0: (0, 1).  A pure host function."""
    from statistics import NormalDist
    k, n = int(k), int(n)
    if not 0 <= k <= n:
        raise ValueError(f"k = {k} outside 0..n = {n}")
    if not 0.0 < level < 1.0:
        raise ValueError(f"level = {level} outside (0, 1)")
    if n == 0:
        return 0.0, 1.0
    z = NormalDist().inv_cdf(1.0 - (1.0 - level) / 2.0)
    p, z2 = k / n, z * z
    centre = p + z2 / (2 * n)
    half = z * np.sqrt(p * (1.0 - p) / n + z2 / (4.0 * n * n))
    lo, hi = (centre - half) / (1.0 + z2 / n), (centre + half) / (1.0 + z2 / n)
    return (0.0 if k == 0 else max(0.0, float(lo))), (1.0 if k == n else min(1.0, float(hi)))


def impact_probability(summary, status=None, engine=None, level=0.95, **kw):
    """The impact probability map of the filtered population (erpl_mc_analyze for the reason bytes, then
    erpl_mc_impact_density on the impact point): the dict of TrajectoryEngine.impact_density - keyword arguments as there
    (nodes, ranges, pad, bandwidth, levels, zones, sample_density, rows) - plus 'n_samples' / 'n_outliers' of the filter
    and, per zone, 'probability' = inside / count with its Wilson score interval 'interval' at `level` ('probability' is
    NaN for an empty population)."""
    engine, res, why = _filter(summary, status, engine)
    out = engine.impact_density(summary, why, **kw)
    out["n_samples"], out["n_outliers"] = int(res.n_valid), int(res.n_outliers)
    out["interval_level"] = float(level)
    for z in out["zones"]:
        z["probability"] = z["inside"] / out["count"] if out["count"] else float("nan")
        z["interval"] = wilson_interval(z["inside"], out["count"], level)
    return out


# ---------------------------------------------------------------------------------- the flight envelope
ENVELOPE_NAMES = ("max_q", "max_q_time", "max_q_altitude", "max_q_mach", "max_mach", "max_q_alpha", "max_axial_acceleration",
                  "min_stability_margin", "max_angular_rate", "max_quaternion_norm_deviation", "burnout_time",
                  "burnout_altitude", "burnout_speed", "burnout_stability_margin", "apogee_record",
                  "usable_records")   # _abi.ENV_* order


def envelope_statistics(envelope, mask=None, engine=None, rows=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95)):
    """Statistics of a flight envelope (float64 [16, m] on the device, TrajectoryEngine.flight_envelope) over the columns
    whose `mask` byte is 0 (uint8 [m] on the device - the reason bytes of the outlier filter; None: every column): the
    kept columns are described by erpl_mc_analyze under infinite bounds, so the order statistics are exact and the sums
    are reduced in its fixed order.  What is left of that filter is its finiteness rule on rows 0, 4 and 5: a column
    whose max_q, max_mach or max_q_alpha is not finite - a trajectory without a usable record - counts in no row; beyond
    that a row counts its finite values (the burnout rows of a flight that ends before burnout are NaN).  rows: _abi.ENV_*
    indices (default all 16).  Returns {name: {'count', 'mean', 'std', 'min', 'max', 'quantiles'}}, names from
    ENVELOPE_NAMES; every number of a row without a counted value is NaN."""
    return _summary_like_statistics(envelope, ENVELOPE_NAMES, mask, engine, rows, quantiles)


def _summary_like_statistics(matrix, names, mask, engine, rows, quantiles):
    """erpl_mc_analyze under infinite bounds on a [16, m] matrix that is laid out like a summary (a flight envelope, an IIP
    summary) over the columns whose mask byte is 0, as {names[r]: {...}}."""
    engine = _engine_of(matrix, engine)
    rows = list(range(len(names))) if rows is None else [int(r) for r in rows]
    quantiles = [float(q) for q in quantiles]
    if mask is not None:
        matrix = matrix[:, mask == 0].contiguous()
    if matrix.shape[1] == 0:
        nan = float("nan")
        return {names[r]: {"count": 0, "mean": nan, "std": nan, "min": nan, "max": nan,
                           "quantiles": [nan] * len(quantiles)} for r in rows}
    inf = float("inf")
    res, _ = engine.analyze(matrix, None, rows=rows, quantiles=quantiles,
                            bounds={"max_apogee": inf, "min_apogee": -inf, "max_range": inf, "max_flight_time": inf,
                                    "energy_apogee": inf})
    return {names[r]: {"count": int(res.row[j].count), "mean": res.row[j].mean, "std": res.row[j].std,
                       "min": res.row[j].min, "max": res.row[j].max,
                       "quantiles": list(res.row[j].quantile[:len(quantiles)])} for j, r in enumerate(rows)}


# ---------------------------------------------------------------------------------- the instantaneous impact points
IIP_NAMES = ("max_range", "max_range_time", "max_range_x", "max_range_y", "burnout_time", "burnout_x", "burnout_y",
             "apogee_x", "apogee_y", "max_rate", "max_rate_time", "exit_time", "exit_x", "exit_y", "landed_nodes",
             "nodes")   # _abi.IIP_* order
IIP_CHANNELS = ("x", "y", "range", "fall_time", "impact_speed")   # _abi.IIP_CH_* order


def impact_point_statistics(summary, mask=None, engine=None, rows=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95)):
    """Statistics of an IIP summary (float64 [16, m] on the device, TrajectoryEngine.impact_points) over the columns whose
    `mask` byte is 0 (uint8 [m] on the device; None: every column), built the way envelope_statistics is: erpl_mc_analyze
    under infinite bounds, exact order statistics, sums in its fixed order.  Its finiteness rule on rows 0, 4 and 5 stays: a
    column whose max_range, burnout_time or burnout_x is not finite - no landed node, a capture that ends before burnout,
    a burnout node that did not land - counts in no row; beyond that a row counts its finite values (the exit rows are
    NaN for a trajectory that stays inside).  rows: _abi.IIP_* indices (default all 16).  Returns
    {name: {'count', 'mean', 'std', 'min', 'max', 'quantiles'}}, names from IIP_NAMES."""
    return _summary_like_statistics(summary, IIP_NAMES, mask, engine, rows, quantiles)


# ---------------------------------------------------------------------------------- the debris footprint
DEBRIS_NAMES = ("max_range", "max_range_time", "max_range_x", "max_range_y", "max_range_fragment", "exit_time", "exit_fragment",
                "exit_x", "exit_y", "max_fall_time", "max_fall_time_time", "max_spread", "max_spread_time", "outside_jobs",
                "landed_jobs", "nodes")   # _abi.DEBRIS_* order
DEBRIS_CHANNELS = IIP_CHANNELS   # the channels of erpl_mc_debris are those of erpl_mc_impact_points


def debris_directions(seed, sample_ids, node, fragment):
    """The break-up directions erpl_mc_debris draws for fragment `fragment` at node `node` of the samples with the global ids
    `sample_ids`: float64 [3, n] (NumPy), unit vectors, the device's bits (erpl_mc_debris_directions_host).  They depend on
    (seed, id, node, fragment) alone.  Needs the library, no GPU."""
    from . import _abi
    lib = _abi.load_library()
    ids = np.ascontiguousarray(sample_ids, dtype=np.int64).reshape(-1)
    out = np.empty((3, len(ids)), dtype=np.float64)
    _abi.check(lib, lib.erpl_mc_debris_directions_host(int(seed) & 0xFFFFFFFFFFFFFFFF, ids.ctypes.data, len(ids), int(node),
                                                       int(fragment), out.ctypes.data), "erpl_mc_debris_directions_host")
    return out


def debris_statistics(summary, mask=None, engine=None, rows=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95)):
    """Statistics of a debris summary (float64 [16, m] on the device, TrajectoryEngine.debris) over the columns whose `mask`
    byte is 0, built the way impact_point_statistics is.  erpl_mc_analyze counts a column only if its rows 0, 4 and 5 are
    finite; row 5 of this summary is exit_time, NaN for every trajectory whose fragments stay inside, so the matrix is handed
    over with rows 5 (exit_time) and 9 (max_fall_time) exchanged: a column counts iff a job of it landed (max_range,
    max_range_fragment and max_fall_time are finite together), and beyond that a row counts its finite values.  rows:
    _abi.DEBRIS_* indices (default all 16).  Returns {name: {'count', 'mean', 'std', 'min', 'max', 'quantiles'}}, names from
    DEBRIS_NAMES."""
    from . import _abi
    swap = list(range(_abi.DEBRIS_DIM))
    swap[_abi.DEBRIS_EXIT_TIME], swap[_abi.DEBRIS_MAX_TFALL] = _abi.DEBRIS_MAX_TFALL, _abi.DEBRIS_EXIT_TIME
    rows = list(range(_abi.DEBRIS_DIM)) if rows is None else [int(r) for r in rows]
    res = _summary_like_statistics(summary[swap].contiguous(), tuple(DEBRIS_NAMES[r] for r in swap), mask, engine,
                                   [swap[r] for r in rows], quantiles)
    return {DEBRIS_NAMES[r]: res[DEBRIS_NAMES[r]] for r in rows}


# ---------------------------------------------------------------------------------- the trajectory corridor
CORRIDOR_CHANNEL_NAMES = ("x", "y", "z", "downrange", "vx", "vy", "vz", "speed")   # _abi.CH_* order


def corridor_channels(channels):
    """Channel names or _abi.CH_* indices as a list of indices."""
    out = []
    for c in channels:
        if isinstance(c, str):
            if c not in CORRIDOR_CHANNEL_NAMES:
                raise ValueError(f"unknown channel {c!r}: one of {CORRIDOR_CHANNEL_NAMES}")
            c = CORRIDOR_CHANNEL_NAMES.index(c)
        out.append(int(c))
    return out


def trajectory_corridor(values, channels=("z", "downrange", "speed"), t0=0.0, dt=1.0,
                        quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), mask=None, engine=None, m=None):
    """The time-resolved bands of a resampled matrix (float64 [C, T, ld] on the device, TrajectoryEngine.corridor_resample
    with these `channels`, `t0` and `dt`) over the columns whose `mask` byte is 0 (uint8 [m] on the device - the reason bytes
    of the outlier filter; None: every column), by one erpl_mc_corridor_bands call.  Returns a dict: 'time' [T] (the nodes
    t0 + k dt), 'q', 'channels' (names), 'n_counted' and, per channel name, {'count', 'mean', 'std', 'min', 'max'} as
    arrays [T] and 'quantiles' [n_q, T]; at a node without a counted finite value every number is NaN."""
    engine = _engine_of(values, engine)
    idx = corridor_channels(channels)
    if len(idx) != int(values.shape[0]):
        raise ValueError(f"{len(idx)} channels for a matrix of {int(values.shape[0])}")
    b = engine.corridor_bands(values, mask, quantiles=quantiles, m=m)
    out = {"time": float(t0) + np.arange(int(values.shape[1]), dtype=np.float64) * float(dt), "q": b["q"],
           "channels": [CORRIDOR_CHANNEL_NAMES[c] for c in idx], "n_counted": b["n_counted"]}
    for j, c in enumerate(idx):
        out[CORRIDOR_CHANNEL_NAMES[c]] = {k: b[k][j] for k in ("count", "mean", "std", "min", "max", "quantiles")}
    return out


def rank_corridor_drivers(pearson, count, factor_names):
    """'share', 'ranking' and 'lead' of `corridor_drivers` from pearson [C, T, F] and count [C, T]: share = pearson^2, the
    linear variance share; per channel the factor names ordered by their largest share over the nodes with count >= 2 (a
    factor without a number there last, ties in factor order); per channel and node the name of the factor with the largest
    share (None where no factor has one)."""
    pearson = np.asarray(pearson, dtype=np.float64)
    share = pearson * pearson
    usable = np.where((np.asarray(count) >= 2)[..., None], share, np.nan)
    ranking, lead = [], []
    for c in range(share.shape[0]):
        some = ~np.all(np.isnan(usable[c]), axis=0)
        best = np.full(share.shape[2], -1.0)
        if usable[c].size:
            best[some] = np.nanmax(usable[c][:, some], axis=0)
        ranking.append([factor_names[f] for f in np.argsort(-best, kind="stable")])
        row = []
        for k in range(share.shape[1]):
            v = usable[c, k]
            row.append(None if np.all(np.isnan(v)) else factor_names[int(np.nanargmax(v))])
        lead.append(row)
    return share, ranking, lead


def corridor_drivers(values, factors, factor_names, channels=None, t0=0.0, dt=1.0, mask=None, engine=None, m=None,
                     regression=True):
    """Which dispersion drives what, and when: for every (channel, node) row of a time-resolved matrix (float64 [C, T, ld] on
    the device - the corridor of TrajectoryEngine.corridor_resample, the matrix of `impact_points` or of `debris`) and every
    row of `factors` (float64 [F, ldf] on the device) the Pearson correlation and the standardised regression coefficient over
    the columns whose `mask` byte is 0 and that are finite in that row - each node has its own population, the flights still
    defined there - by one erpl_mc_corridor_drivers call.  channels: the names of the C channels (default 'channel 0' ..).
    Returns the dict of TrajectoryEngine.corridor_drivers plus 'time' [T] (t0 + k dt), 'channels', 'factor_names', 'share'
    (pearson^2 [C, T, F], the linear variance share), 'ranking' (per channel the factor names by their largest share over
    the nodes with count >= 2) and 'lead' (per channel and node the leading factor's name, None where there is none)."""
    engine = _engine_of(values, engine)
    factor_names = list(factor_names)
    if len(factor_names) != int(factors.shape[0]):
        raise ValueError(f"{len(factor_names)} factor names for {int(factors.shape[0])} factor rows")
    if values.dim() != 3:
        raise ValueError("values must be a [C, T, ld] matrix")
    n_ch, n_nodes = int(values.shape[0]), int(values.shape[1])
    channels = [f"channel {c}" for c in range(n_ch)] if channels is None else \
        [CORRIDOR_CHANNEL_NAMES[c] if not isinstance(c, str) else c for c in channels]
    if len(channels) != n_ch:
        raise ValueError(f"{len(channels)} channels for a matrix of {n_ch}")
    out = engine.corridor_drivers(factors, values, mask=mask, m=m, regression=regression)
    out["time"] = float(t0) + np.arange(n_nodes, dtype=np.float64) * float(dt)
    out["channels"], out["factor_names"] = channels, factor_names
    out["share"], out["ranking"], out["lead"] = rank_corridor_drivers(out["pearson"], out["count"], factor_names)
    return out


def outliergram(depth, mei, n):
    """The shape outliers of Arribas-Gil & Romo (2014) from the modified band depth and the modified epigraph index of curves
    that share one population of n at every node: a curve that crosses no other lies ON the parabola
    depth = a0 + a1 mei + a2 n^2 mei^2 with a0 = a2 = -2 / (n (n - 1)) and a1 = 2 (n + 1) / (n - 1), a curve that crosses many
    lies below it.  Returns (d, flags): d = the parabola minus depth (NaN where depth or mei is), flags = d > Q3 + 1.5 IQR over
    the finite distances - and d > 1e-13, so that the rounding of curves that cross nothing (|d| of a few 1e-15) flags none."""
    depth, mei = np.asarray(depth, dtype=np.float64), np.asarray(mei, dtype=np.float64)
    n = float(n)
    if n < 2:
        return np.full(depth.shape, np.nan), np.zeros(depth.shape, dtype=bool)
    a0 = a2 = -2.0 / (n * (n - 1.0))
    a1 = 2.0 * (n + 1.0) / (n - 1.0)
    d = a0 + a1 * mei + a2 * n * n * mei * mei - depth
    ok = np.isfinite(d)
    if not ok.any():
        return d, np.zeros(depth.shape, dtype=bool)
    q1, q3 = np.quantile(d[ok], (0.25, 0.75))
    with np.errstate(invalid="ignore"):
        return d, ok & (d > q3 + 1.5 * (q3 - q1)) & (d > 1e-13)


def trajectory_depth(values, channels=None, t0=0.0, dt=1.0, mask=None, engine=None, central=0.5, factor=1.5, m=None, lds_limit=0):
    """Which flown trajectory is the typical one and which flights are unusual as curves: the modified band depth, the
    functional boxplot and the outliergram of a time-resolved matrix (float64 [C, T, ld] on the device - the corridor of
    TrajectoryEngine.corridor_resample, the matrix of `impact_points` or of `debris`) over the columns whose `mask` byte is 0,
    by one erpl_mc_corridor_depth call per matrix.  channels: the names of the C channels (default 'channel 0' ..).
    Returns a dict: 'time' [T] (t0 + k dt), 'channels', 'central_share', 'factor', 'n_masked', 'warnings' and per channel name
    {'depth', 'mei' [m] (NumPy), 'nodes' [m], 'median' (the deepest column, -1 if none), 'median_curve' [T] (that column of
    the matrix), 'central', 'fence', 'whisker' (each {'lo', 'hi'} [T]), 'count' [T], 'n_defined', 'n_central',
    'magnitude_outliers' (the columns that leave the fences: a list of {'column', 'first_node', 'nodes'}), 'shape_outliers'
    (the columns the outliergram flags, with 'outliergram_distance' [m]) - the outliergram needs one population at every
    counted node of the channel (a matrix resampled with hold=True over flights that ran to their end); where the populations
    differ 'shape_outliers' is None and 'warnings' says so}."""
    engine = _engine_of(values, engine)
    if values.dim() != 3:
        raise ValueError("values must be a [C, T, ld] matrix")
    n_ch, n_nodes = int(values.shape[0]), int(values.shape[1])
    channels = [f"channel {c}" for c in range(n_ch)] if channels is None else \
        [CORRIDOR_CHANNEL_NAMES[c] if not isinstance(c, str) else c for c in channels]
    if len(channels) != n_ch:
        raise ValueError(f"{len(channels)} channels for a matrix of {n_ch}")
    r = engine.corridor_depth(values, mask=mask, m=m, central=central, factor=factor, lds_limit=lds_limit)
    out = {"time": float(t0) + np.arange(n_nodes, dtype=np.float64) * float(dt), "channels": channels,
           "central_share": float(central), "factor": float(factor), "n_masked": r["n_masked"], "warnings": []}
    cols = {k: r[k].cpu().numpy() for k in ("depth", "mei", "nodes", "n_out", "first_out")}
    for c, name in enumerate(channels):
        med = int(r["median"][c])
        ch = {"depth": cols["depth"][c], "mei": cols["mei"][c], "nodes": cols["nodes"][c], "median": med,
              "median_curve": values[c, :, med].cpu().numpy() if med >= 0 else np.full(n_nodes, np.nan),
              "central": {"lo": r["central_lo"][c], "hi": r["central_hi"][c]},
              "fence": {"lo": r["fence_lo"][c], "hi": r["fence_hi"][c]},
              "whisker": {"lo": r["whisker_lo"][c], "hi": r["whisker_hi"][c]},
              "count": r["count"][c], "n_defined": int(r["n_defined"][c]), "n_central": int(r["n_central"][c]),
              "threshold": float(r["threshold"][c])}
        defined = cols["nodes"][c] > 0
        ch["magnitude_outliers"] = [{"column": int(j), "first_node": int(cols["first_out"][c][j]), "nodes": int(cols["n_out"][c][j])}
                                    for j in np.flatnonzero(defined & (cols["n_out"][c] > 0))]
        counted = r["count"][c][r["count"][c] >= 2]
        same = len(counted) > 0 and np.all(counted == counted[0]) and np.all(cols["nodes"][c][defined] == len(counted))
        if same:
            d, flags = outliergram(np.where(defined, ch["depth"], np.nan), ch["mei"], int(counted[0]))
            ch["outliergram_distance"], ch["shape_outliers"] = d, [int(j) for j in np.flatnonzero(flags)]
        else:
            ch["outliergram_distance"], ch["shape_outliers"] = None, None
            out["warnings"].append(f"{name}: the populations of the nodes differ, no outliergram (resample with hold=True)")
        out[name] = ch
    return out


# ---------------------------------------------------------------------------------- drivers: which dispersion drives what
ROW_NAMES = ("apogee_altitude", "apogee_time", "first_apogee_altitude", "first_apogee_time", "range", "flight_time",
             "rail_exit_time", "rail_exit_speed", "impact_x", "impact_y", "impact_z", "n_steps",
             "rail_exit_angle_of_attack", "rail_exit_sideslip", "final_vz", "max_speed")   # _abi.SUM_* order

_VEC_PARAMS = ("initial_position_offset", "initial_velocity_offset", "initial_attitude_offset",
               "initial_angular_velocity_offset")
_SCALAR_PARAMS = ("mass_multiplier", "thrust_multiplier", "wind_speed", "wind_direction", "density_multiplier")
_MOTOR_INPUTS = ("motor_thrust", "motor_mass_flow_rate")


def factors_from_results(results):
    """The reference's per-sample `parameters` dicts (monte_carlo.py:156-179) of a list of result records as factor rows:
    (float64 [F, n] NumPy array, names).  Names: `initial_position_offset[0]` ... `initial_angular_velocity_offset[2]`,
    then mass_multiplier, thrust_multiplier, wind_speed, wind_direction, density_multiplier - `random_seed` is left out;
    thrust_multiplier and density_multiplier, which the reference draws and then ignores, are kept on purpose: a
    parameter without effect showing a correlation of about 0 is information - and, where the records carry
    `motor_inputs`, the two motor inputs the kernel actually saw: motor_thrust and motor_mass_flow_rate.  A key that a
    record does not carry is NaN there (listwise deletion then drops the sample)."""
    records = [r for r in results if r is not None]
    names = [f"{k}[{c}]" for k in _VEC_PARAMS for c in range(3)] + list(_SCALAR_PARAMS)
    with_motor = any("motor_inputs" in r for r in records)
    if with_motor:
        names += list(_MOTOR_INPUTS)
    out = np.full((len(names), len(records)), np.nan)
    for i, r in enumerate(records):
        p = r.get("parameters", {})
        for j, k in enumerate(_VEC_PARAMS):
            if k in p:
                out[3 * j:3 * j + 3, i] = np.asarray(p[k], dtype=np.float64)
        for j, k in enumerate(_SCALAR_PARAMS):
            if k in p:
                out[12 + j, i] = p[k]
        if with_motor:
            m = r.get("motor_inputs", {})
            for j, k in enumerate(_MOTOR_INPUTS):
                out[12 + len(_SCALAR_PARAMS) + j, i] = m.get(k, np.nan)
    return out, names


def summary_from_results(results):
    """The [16, n] summary columns behind a list of result records (rows a record does not carry are NaN)."""
    from . import _abi
    from .results import SCALAR_COLUMNS
    table, ids = getattr(results, "table", None), getattr(results, "ids", None)
    if table is not None and ids is not None:
        return np.ascontiguousarray(table.summary[:, ids], dtype=np.float64)
    records = [r for r in results if r is not None]
    cols = np.full((_abi.SUMMARY_DIM, len(records)), np.nan)
    for i, r in enumerate(records):
        for name, row in SCALAR_COLUMNS:
            cols[row, i] = r.get(name, np.nan)
        if r.get("impact_position") is not None:
            cols[_abi.SUM_IMPACT_X:_abi.SUM_IMPACT_Z + 1, i] = r["impact_position"]
        cols[_abi.SUM_STEPS, i] = r.get("n_steps", np.nan)
    return cols


def rank_drivers(corr, factor_names, ranks=True):
    """For every row of a correlation dict the factor names sorted by |spearman| descending (|pearson| when
    ranks=False), constant factors (NaN) last, ties and the constant ones in factor order."""
    rho = np.abs(np.asarray(corr["spearman" if ranks else "pearson"], dtype=np.float64))
    out = []
    for j in range(rho.shape[0]):
        key = np.where(np.isnan(rho[j]), -1.0, rho[j])
        out.append([factor_names[f] for f in np.argsort(-key, kind="stable")])
    return out


def drivers(summary, factors, factor_names, status=None, engine=None, rows=None, ranks=True):
    """Which input dispersion drives which outcome, on the device: erpl_mc_analyze for the reason bytes (as
    `native_distributions`), then erpl_mc_correlation between the rows of `factors` (float64 [F, n] device tensor, e.g.
    `run_monte_carlo_device(..., keep_factors=True)['factors']`) and summary rows `rows` (default apogee, range, flight
    time) over the samples the filter keeps and whose factors and rows are all finite.  Returns the dict of
    TrajectoryEngine.correlation plus 'factor_names', 'row_names', 'n_samples', 'n_outliers' and 'ranking': per row the
    factor names by |spearman| descending (|pearson| when ranks=False), constant factors last.

    Reading it: spearman / pearson are marginal, srrc / src are the effect with the other factors held fixed and
    r2_rank / r2 say how much of the outcome the (rank-)linear model explains.  Factors that are affine images of one
    another (see `sampling.synthetic_dispersions`: position_x and motor_thrust_multiplier with a non-zero position
    sigma) cannot be separated: regression_ok = 0 and the coefficients are NaN, the correlations stay."""
    engine = _engine_of(summary, engine)   # (a missing GPU is reported before a wrong list of names)
    factor_names = list(factor_names)
    if len(factor_names) != int(factors.shape[0]):
        raise ValueError(f"{len(factor_names)} factor names for {int(factors.shape[0])} factor rows")
    engine, res, why = _filter(summary, status, engine)
    out = engine.correlation(factors, summary, why, rows=rows, ranks=ranks)
    out["factor_names"] = factor_names
    out["row_names"] = [ROW_NAMES[r] for r in out["rows"]]
    out["n_samples"], out["n_outliers"] = int(res.n_valid), int(res.n_outliers)
    out["ranking"] = rank_drivers(out, factor_names, ranks)
    return out


# ---------------------------------------------------------------------------------- how sure the statistics are
def bootstrap_indices(seed, replicate, m, first=0, count=None):
    """The dense population indices (int64 NumPy array) replicate `replicate` of a bootstrap with `seed` draws from a
    population of m, draws first .. first + count - 1 (default: all m): erpl_mc_bootstrap_indices, the host copy of the
    device's draws.  Dense index d is the d-th sample, in sample order, that the filter keeps and whose requested rows are
    all finite.  Needs the library, no GPU."""
    from . import _abi
    lib = _abi.load_library()
    m, first = int(m), int(first)
    count = m - first if count is None else int(count)
    out = np.empty(max(count, 0), dtype=np.int64)
    _abi.check(lib, lib.erpl_mc_bootstrap_indices(int(seed) & 0xFFFFFFFFFFFFFFFF, int(replicate), m, first, count,
                                                  out.ctypes.data), "erpl_mc_bootstrap_indices")
    return out


def _interval(s):
    return {k: s[k] for k in ("estimate", "se", "lo", "hi")}


def confidence_intervals(summary, status=None, engine=None, rows=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95),
                         replicates=2000, level=0.95, seed=0, extra=None):
    """Bootstrap confidence intervals of the statistics `native_statistics` reports, on the device: erpl_mc_analyze for
    the reason bytes, then erpl_mc_bootstrap over the samples that carry none.  rows: up to 4 summary rows (default
    apogee, range, flight time).  Returns, per row name (ROW_NAMES), {'mean': {estimate, se, lo, hi}, 'std': {..},
    'percentiles': [{..}, ..]} - se the bootstrap standard error, (lo, hi) the `level` percentile interval - plus
    'n_samples', 'n_outliers', 'count' (the population: kept and finite in every row), 'quantiles', 'level',
    'replicates' and 'seed'.

    The bootstrap assumes i.i.d. columns.  The columns of a Latin hypercube run (run_monte_carlo_device(design='lhs')) are
    not: they are negatively dependent, the mean of a near-additive output varies far less than resampling its columns
    suggests, and these intervals are conservative (too wide) for such a run.  Its valid error bar comes from independent
    replicates of the design: `replicate_intervals`.

    extra: a float64 [n] device tensor of one more value per sample (the 'ec_traj' of `casualty_expectation`, say); it joins
    the rows as _abi.BOOT_ROW_EXTRA - by default behind apogee, range and flight time - and is reported under 'extra'."""
    from . import _abi
    engine, res, why = _filter(summary, status, engine)
    if extra is not None and rows is None:
        rows = (_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, _abi.BOOT_ROW_EXTRA)
    b = engine.bootstrap(summary, why, rows=rows, quantiles=quantiles, replicates=replicates, level=level, seed=seed, extra=extra)
    name_of = lambda r: ROW_NAMES[r] if r < len(ROW_NAMES) else "extra"   # noqa: E731
    out = {name_of(r): {"mean": _interval(s["mean"]), "std": _interval(s["std"]),
                          "percentiles": [_interval(p) for p in s["quantiles"]]} for r, s in zip(b["rows"], b["stats"])}
    out["n_samples"], out["n_outliers"], out["count"] = int(res.n_valid), int(res.n_outliers), b["count"]
    out["quantiles"], out["level"], out["replicates"], out["seed"] = b["q"], b["level"], b["replicates"], b["seed"]
    return out


def replicate_intervals(summary, status, block, rows=None, level=0.95, engine=None):
    """The error bar of a replicated design run (run_monte_carlo_device(design=..., design_replicates=R) with
    block = n_samples / R): the columns [j block, (j + 1) block) of `summary` are R independent replicates of one design,
    so the R replicate means of a row are i.i.d. whatever the dependence inside a replicate.  Per requested row (default
    apogee, range, flight time) the mean of every replicate through erpl_mc_analyze on that column slice - outliers
    filtered and non-finite values dropped as everywhere - and across the replicates the mean of means, its standard error
    s / sqrt(R) (s with R - 1 in the denominator) and the Student-t interval at `level` with R - 1 degrees of freedom.
    Returns, per row name (ROW_NAMES), {'replicate_means': [..], 'replicate_counts': [..], 'mean', 'se', 'lo', 'hi'}, plus
    'replicates', 'block' and 'level'.  R = 1: se, lo and hi are NaN, one hypercube has no error bar of its own.
    The replicates of design='qmc' are independently scrambled nets and this is their error bar too; the bootstrap
    (`bootstrap_intervals`) is no more valid for the columns of a net than for those of a hypercube."""
    from scipy import stats as sps

    from . import _abi
    engine = _engine_of(summary, engine)
    n, block = int(summary.shape[1]), int(block)
    if block < 1 or n % block != 0:
        raise ValueError(f"block = {block} does not divide the {n} columns of the summary")
    if not 0.0 < float(level) < 1.0:
        raise ValueError("level must lie in (0, 1)")
    rows = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME] if rows is None else [int(r) for r in rows]
    R = n // block
    means, counts = np.empty((len(rows), R)), np.empty((len(rows), R), dtype=np.int64)
    for j in range(R):
        cols = slice(j * block, (j + 1) * block)
        res, _ = engine.analyze(summary[:, cols].contiguous(), None if status is None else status[cols].contiguous(),
                                rows=rows, quantiles=[])
        for i in range(len(rows)):
            means[i, j], counts[i, j] = res.row[i].mean, res.row[i].count
    out = {"replicates": R, "block": block, "level": float(level)}
    for i, r in enumerate(rows):
        mean = float(np.mean(means[i]))
        se = float(np.std(means[i], ddof=1) / np.sqrt(R)) if R > 1 else float("nan")
        half = float(sps.t.ppf(0.5 + 0.5 * float(level), R - 1)) * se if R > 1 else float("nan")
        out[ROW_NAMES[r]] = {"replicate_means": means[i].tolist(), "replicate_counts": counts[i].tolist(), "mean": mean,
                             "se": se, "lo": mean - half, "hi": mean + half}
    return out


def cep_interval(summary, status=None, engine=None, target=None, quantiles=(0.5, 0.9, 0.95, 0.99), replicates=2000,
                 level=0.95, seed=0):
    """The CEP with its confidence interval: erpl_mc_analyze for the reason bytes, erpl_mc_dispersion for the miss distance
    about `target` ((x, y), default the launch site) of every sample, then erpl_mc_bootstrap on that row (`extra`) with the
    dispersion's quantile fractions.  Returns {'cep': {estimate, se, lo, hi} or None without 0.5 among the quantiles,
    'quantiles': [{..}, ..] in the order of `quantiles`, 'mean': {..}, 'std': {..}, 'q', 'count', 'n_samples',
    'n_outliers', 'level', 'replicates', 'seed'}; the estimates are the bits `landing_dispersion` reports."""
    from . import _abi
    engine, res, why = _filter(summary, status, engine)
    quantiles = [float(q) for q in quantiles]
    disp = engine.dispersion(summary, why, centre=(0.0, 0.0) if target is None else target, quantiles=quantiles, miss=True)
    b = engine.bootstrap(summary, why, rows=[_abi.BOOT_ROW_EXTRA], quantiles=quantiles, replicates=replicates, level=level,
                         seed=seed, extra=disp["miss_distance"])
    s = b["stats"][0]
    qs = [_interval(p) for p in s["quantiles"]]
    return {"cep": qs[quantiles.index(0.5)] if 0.5 in quantiles else None, "quantiles": qs, "mean": _interval(s["mean"]),
            "std": _interval(s["std"]), "q": quantiles, "count": b["count"], "n_samples": int(res.n_valid),
            "n_outliers": int(res.n_outliers), "level": b["level"], "replicates": b["replicates"], "seed": b["seed"]}


# ---------------------------------------------------------------------------------- variance-based sensitivity
def rank_total_effects(total, group_names):
    """For every row of `total` ([R, k] total-effect indices) the group names by ST descending, NaN last, ties and the NaN
    ones in group order."""
    total = np.asarray(total, dtype=np.float64)
    out = []
    for j in range(total.shape[0]):
        key = np.where(np.isnan(total[j]), -np.inf, total[j])
        out.append([group_names[f] for f in np.argsort(-key, kind="stable")])
    return out


def sobol_indices(summary, n_base, group_names, mask=None, engine=None, rows=None, extra=None, replicates=1000, level=0.95,
                  seed=0):
    """First-order and total-effect Sobol indices of a pick-freeze run, on the device (TrajectoryEngine.sobol,
    erpl_mc_sobol): `summary` is the float64 [16, (k + 2) n_base] device tensor of the design flown block by block - A, B,
    then A with group i taken from B for every name of `group_names` (MonteCarloAnalyzer.sobol_indices flies it).  mask:
    uint8 [n_base] device tensor, byte 0 = the design row counts.  Returns the engine's dict plus 'group_names',
    'row_names', 'ranking' (per row the group names by total effect descending, NaN last), 'sum_first' ([R], the sum of
    the first-order estimates) and 'interaction' = 1 - sum_first: the share of the variance no factor explains alone.

    Reading it: first[i] is the share of the output's variance that fixing group i alone would remove, total[i] the share
    that remains while everything BUT group i is fixed - interactions included, which no regression coefficient sees.
    total = 0 exactly: the group does not reach the output at all."""
    engine = _engine_of(summary, engine)
    group_names = [str(g) for g in group_names]
    out = engine.sobol(summary, n_base, len(group_names), mask=mask, rows=rows, extra=extra, replicates=replicates,
                       level=level, seed=seed)
    out["group_names"] = group_names
    out["row_names"] = ["extra" if r >= len(ROW_NAMES) else ROW_NAMES[r] for r in out["rows"]]
    out["ranking"] = rank_total_effects(out["total"]["estimate"], group_names)
    out["sum_first"] = out["first"]["estimate"].sum(axis=1)
    out["interaction"] = 1.0 - out["sum_first"]
    return out


# ---------------------------------------------------------------------------------- given-data sensitivity of an ordinary run
DEP_MEASURES = ("delta", "ks_max", "ks_median", "mi")


def given_data_sensitivity(summary, factors, factor_names, status=None, engine=None, rows=None, extra=None, classes=16, cells=16,
                           shifts=200, level=0.95, seed=0, want_tables=False, want_null=False):
    """Which input dispersion drives which outcome without assuming a linear or monotone response, from the run you
    already have: erpl_mc_analyze for the reason bytes (as `drivers`), then erpl_mc_dependence (TrajectoryEngine.dependence)
    between the rows of `factors` (float64 [F, n] device tensor, e.g. `run_monte_carlo_device(..., keep_factors=True)
    ['factors']`) and up to 4 summary rows `rows` (default apogee, range, flight time) over the samples the filter keeps
    and whose factors and rows are all finite.  Returns the dict of TrajectoryEngine.dependence plus 'factor_names',
    'row_names', 'n_samples', 'n_outliers'; per measure (delta, ks_max, ks_median, mi) 'p_value' = (exceed + 1) / (shifts
    + 1) and 'excess' = max(0, estimate - null_mean) (NaN without shifts); 'ranking': per row the factor names by the
    excess of delta descending (by delta itself without shifts), NaN last; and 'curves': per row and factor {'x', 'mean',
    'std', 'count'} over the non-empty classes - the class centres x_median with the conditional mean and std of the
    outcome, the main-effect curve.

    Reading it: eta2 is the first-order Sobol index of a factor that is independent of the others - the share of the
    outcome's variance its conditional mean explains, non-monotone effects included (Spearman reads about 0 for wind
    direction, eta2 does not).  Under the default joint law of `sampling.synthetic_dispersions` entangled factors
    (position_x and motor_thrust_multiplier share a normal) share their effect, as they do in `drivers`.  delta, KS and
    mi also see a factor that changes only the SHAPE of the outcome's distribution (Ishigami's x3: eta2 = 0, delta about
    0.13), but are biased upwards at finite n: compare every one with its null band.  A measure inside the band (estimate
    <= null_hi, p_value not small) is indistinguishable from "no effect" at this n."""
    engine = _engine_of(summary, engine)
    factor_names = list(factor_names)
    if len(factor_names) != int(factors.shape[0]):
        raise ValueError(f"{len(factor_names)} factor names for {int(factors.shape[0])} factor rows")
    engine, res, why = _filter(summary, status, engine)
    out = engine.dependence(factors, summary, why, rows=rows, extra=extra, classes=classes, cells=cells, shifts=shifts,
                            level=level, seed=seed, want_tables=want_tables, want_curves=True, want_null=want_null)
    out["factor_names"] = factor_names
    out["row_names"] = [ROW_NAMES[r] if r < len(ROW_NAMES) else "extra" for r in out["rows"]]
    out["n_samples"], out["n_outliers"] = int(res.n_valid), int(res.n_outliers)
    finish_given_data(out)
    return out


def finish_given_data(out):
    """What `given_data_sensitivity` adds to the dict of TrajectoryEngine.dependence that needs no device: p_value and
    excess of every measure, 'ranking' and 'curves' (in place)."""
    P = int(out["shifts"])
    for key in DEP_MEASURES:
        m = out[key]
        est, mean = np.asarray(m["estimate"], dtype=np.float64), np.asarray(m["null_mean"], dtype=np.float64)
        have = P > 0 and int(out["count"]) >= 2
        m["p_value"] = (np.asarray(m["exceed"]) + 1.0) / (P + 1.0) if have else np.full(est.shape, np.nan)
        m["excess"] = np.maximum(0.0, est - mean) if have else np.full(est.shape, np.nan)
    names = out["factor_names"]
    score = out["delta"]["excess"] if np.isfinite(out["delta"]["excess"]).any() else np.asarray(out["delta"]["estimate"])
    out["ranking"] = []
    for j in range(score.shape[0]):
        key = np.where(np.isnan(score[j]), -1.0, score[j])
        out["ranking"].append([names[f] for f in np.argsort(-key, kind="stable")])
    cs = np.asarray(out["class_stats"], dtype=np.float64)
    out["curves"] = []
    for j in range(cs.shape[0]):
        per_factor = {}
        for f, name in enumerate(names):
            used = cs[j, f, :, 0] > 0
            per_factor[name] = {"x": cs[j, f, used, 5], "mean": cs[j, f, used, 1], "std": cs[j, f, used, 2],
                                "count": cs[j, f, used, 0].astype(np.int64)}
        out["curves"].append(per_factor)
    return out


# ---------------------------------------------------------------------------------- polynomial chaos surrogate
def surrogate_terms(n_vars, degree, order):
    """The terms of the polynomial chaos basis of erpl_mc_surrogate (host only, no device): int8 [P, 4, 2], per term the
    (variable, degree) of its up to 4 factors in ascending variable order, unused slots (-1, 0); term 0 is the constant."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    P = C.c_int32(0)
    _abi.check(lib, lib.erpl_mc_surrogate_terms(int(n_vars), int(degree), int(order), C.byref(P), None), "erpl_mc_surrogate_terms")
    terms = np.empty((P.value, 4, 2), dtype=np.int8)
    _abi.check(lib, lib.erpl_mc_surrogate_terms(int(n_vars), int(degree), int(order), C.byref(P), C.c_void_p(terms.ctypes.data)),
               "erpl_mc_surrogate_terms")
    return terms


def polynomial_chaos(summary, factors, kinds, names, status=None, engine=None, rows=None, extra=None, degree=2, order=2, holdout=5,
                     top=10):
    """A polynomial chaos surrogate of a run of INDEPENDENT primitives (a run flown with design=...): erpl_mc_analyze for
    the reason bytes (as `drivers`), then erpl_mc_surrogate (TrajectoryEngine.surrogate) of the rows of `factors` (float64
    [V, n] device tensor of primitives, `kinds` their laws) on up to 4 summary rows over the samples the filter keeps.
    Returns the dict of TrajectoryEngine.surrogate plus 'names', 'row_names', 'n_samples', 'n_outliers', 'ranking' (per row
    the variable names by total index descending, NaN last) and 'interactions' (per row the `top` largest pair indices as
    (name_i, name_j, index), descending).

    Reading it: first / total / pair are shares of the variance the surrogate EXPLAINS; r2 is the share of the outcome's
    variance the chosen variables explain at all (the turbulence rows of a flight are not among them), q2 the same on the
    members held out of the fit - trust the indices and the emulator as far as q2 goes."""
    engine = _engine_of(summary, engine)
    names = list(names)
    if len(names) != int(factors.shape[0]):
        raise ValueError(f"{len(names)} names for {int(factors.shape[0])} variable rows")
    engine, res, why = _filter(summary, status, engine)
    out = engine.surrogate(factors, kinds, summary, why, rows=rows, extra=extra, degree=degree, order=order, holdout=holdout)
    out["names"] = names
    out["row_names"] = [ROW_NAMES[r] if r < len(ROW_NAMES) else "extra" for r in out["rows"]]
    out["n_samples"], out["n_outliers"] = int(res.n_valid), int(res.n_outliers)
    if out["n_val"] > 0:   # predicted against flown on (at most 4096 of) the held-out members, for the plot
        import torch
        from . import _abi
        pred = engine.surrogate_predict(out["model"], factors)
        y = torch.stack([extra if r == _abi.SUR_ROW_EXTRA else summary[r] for r in out["rows"]])
        members = torch.nonzero((why == 0) & torch.isfinite(factors).all(0) & torch.isfinite(y).all(0)).flatten()
        held = members[holdout - 1::holdout][:4096]
        out["validation"] = {"samples": held.cpu().numpy(), "flown": y[:, held].cpu().numpy(),
                             "predicted": pred[:, held].cpu().numpy()}
    return finish_polynomial_chaos(out, top)


def finish_polynomial_chaos(out, top=10):
    """What `polynomial_chaos` adds to the dict of TrajectoryEngine.surrogate that needs no device: 'ranking' and
    'interactions' (in place)."""
    names = out["names"]
    V = len(names)
    out["ranking"], out["interactions"] = [], []
    for j in range(len(out["rows"])):
        total = np.asarray(out["total"][j], dtype=np.float64)
        out["ranking"].append([names[v] for v in np.argsort(-np.where(np.isnan(total), -1.0, total), kind="stable")])
        pair = np.asarray(out["pair"][j], dtype=np.float64)
        found = [(pair[a, b], a, b) for a in range(V) for b in range(a + 1, V) if np.isfinite(pair[a, b])]
        found.sort(key=lambda e: -e[0])
        out["interactions"].append([(names[a], names[b], float(v)) for v, a, b in found[:top]])
    return out


# ---------------------------------------------------------------------------------- two runs: the same law?
def permutation_labels(seed, permutation, m_a, m_b):
    """Side A (True) of permutation `permutation` of erpl_mc_compare with `seed`, for m_a + m_b pooled members (A's counted
    samples in sample order, then B's): erpl_mc_compare_labels, the host copy of the device's labels.  Exactly m_a are
    True.  Needs the library, no GPU."""
    from . import _abi
    lib = _abi.load_library()
    out = np.empty(max(int(m_a) + int(m_b), 0), dtype=np.uint8)
    _abi.check(lib, lib.erpl_mc_compare_labels(int(seed) & 0xFFFFFFFFFFFFFFFF, int(permutation), int(m_a), int(m_b),
                                               out.ctypes.data), "erpl_mc_compare_labels")
    return out.astype(bool)


COMPARE_TESTS = (("ks", "Kolmogorov-Smirnov"), ("mw", "Mann-Whitney"), ("cvm", "Cramer-von Mises"))


def compare_runs(a, b, status_a=None, status_b=None, engine=None, **kw):
    """Two runs side by side: each summary ([16, n] float64 on the device, with its status or None, as `native_statistics`
    takes them) goes through the outlier filter of erpl_mc_analyze, then erpl_mc_compare tests the two filtered populations
    (keywords of TrajectoryEngine.compare: rows, quantiles, xy, permutations, level, seed, keep_null, extra_a, extra_b).
    Returns that dict plus 'n_samples_a' / 'n_samples_b' / 'n_outliers_a' / 'n_outliers_b', per row 'name', 'p_values'
    ({ks, mw, cvm}) and 'verdict', and 'energy_verdict': one line each, at 1 - level.  Without permutations there are no
    p-values and the verdicts say so."""
    engine, res_a, why_a = _filter(a, status_a, engine)
    _, res_b, why_b = _filter(b, status_b, engine)
    out = engine.compare(a, b, mask_a=why_a, mask_b=why_b, **kw)
    out["n_samples_a"], out["n_samples_b"] = int(res_a.n_valid), int(res_b.n_valid)
    out["n_outliers_a"], out["n_outliers_b"] = int(res_a.n_outliers), int(res_b.n_outliers)
    return finish_comparison(out)


def finish_comparison(out):
    """Row names, p-values and the one-line verdicts of a TrajectoryEngine.compare dict (in place; returns it)."""
    alpha = 1.0 - out["level"]
    tested = out["permutations"] > 0 and out["count_a"] > 0 and out["count_b"] > 0
    for r, row in zip(out["rows"], out["row"]):
        row["name"] = ROW_NAMES[r] if 0 <= r < len(ROW_NAMES) else "extra"
        row["p_values"] = {k: row[k]["p_value"] for k, _ in COMPARE_TESTS}
        if not tested:
            row["verdict"] = f"{row['name']}: not tested (no permutations or an empty run)"
            continue
        hit = [full for k, full in COMPARE_TESTS if row[k]["p_value"] <= alpha]
        shift = row["mean_b"] - row["mean_a"]
        row["verdict"] = (f"{row['name']}: differs at {alpha:.3g} ({', '.join(hit)}; mean shift {shift:+.6g}, "
                          f"P(A > B) = {row['prob_superiority']:.3f})" if hit else
                          f"{row['name']}: no difference at {alpha:.3g} (smallest p = {min(row['p_values'].values()):.3g})")
    e = out.get("energy")
    if e is None:
        out["energy_verdict"] = "impact clouds: not tested"
    elif not tested:
        out["energy_verdict"] = f"impact clouds: E = {e['statistic']:.6g}, not tested (no permutations)"
    else:
        out["energy_verdict"] = (f"impact clouds: {'differ' if e['p_value'] <= alpha else 'no difference'} at {alpha:.3g} "
                                 f"(E = {e['statistic']:.6g}, null {100 * out['level']:.0f} % = {e['null_hi']:.6g}, "
                                 f"p = {e['p_value']:.3g})")
    return out


# ---------------------------------------------------------------------------------- the tally: a run in bounded memory
def _row_id(row):
    """A summary row by its name (ROW_NAMES) or its _abi.SUM_* index."""
    if isinstance(row, str):
        if row not in ROW_NAMES:
            raise ValueError(f"unknown summary row {row!r}: one of {ROW_NAMES}")
        return ROW_NAMES.index(row)
    return int(row)


def tally_spec(rows=None, ranges=None, bins=None, centres=None, thresholds=None, k=None, quantiles=None, bounds=None,
               grid_rows=None, grid_bins=None, grid_ranges=None, zones=None):
    """The spec of a tally (erpl_mc_tally_*; _abi.ErplTallySpec) from keyword arguments, every one of them optional on top of
    the library's defaults (erpl_mc_tally_defaults: apogee 0..80 km, range 0..200 km, flight time 0..600 s, 1000 bins,
    k = 16, the impact point on 128 x 128 cells over +-200 km).  A pure host function.
    rows: up to 8 summary rows by name (ROW_NAMES) or index; with rows given, ranges is required: one (lo, hi) per row
    (streaming has no range from the data).  bins: one int or one per row; centres: one per row (default mid-range);
    thresholds: {row: [values]} or one list per row; k: extremes held per row and side (0..64); quantiles: fractions in
    [0, 1]; bounds: the dict of TrajectoryEngine.analyze; grid_rows: (row_x, row_y); grid_bins: one int or (bins_x, bins_y);
    grid_ranges: ((lo_x, hi_x), (lo_y, hi_y)); zones: polygons, each an array of (x, y) vertices."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    spec = _abi.ErplTallySpec()
    _abi.check(lib, lib.erpl_mc_tally_defaults(C.byref(spec)), "erpl_mc_tally_defaults")
    if rows is not None:
        rows = [_row_id(r) for r in rows]
        if len(rows) > _abi.TALLY_MAX_ROWS:
            raise ValueError(f"at most {_abi.TALLY_MAX_ROWS} rows")
        if ranges is None or len(ranges) != len(rows):
            raise ValueError("ranges: one (lo, hi) per row - a tally has no range from the data")
        spec.n_rows = len(rows)
        for j, r in enumerate(rows):
            spec.rows[j], spec.bins[j], spec.n_thresholds[j] = r, 1000, 0
            spec.lo[j], spec.hi[j] = float(ranges[j][0]), float(ranges[j][1])
            spec.centre[j] = 0.5 * (spec.lo[j] + spec.hi[j])
    elif ranges is not None:
        if len(ranges) != spec.n_rows:
            raise ValueError("ranges: one (lo, hi) per row")
        for j, (lo, hi) in enumerate(ranges):
            spec.lo[j], spec.hi[j] = float(lo), float(hi)
            spec.centre[j] = 0.5 * (spec.lo[j] + spec.hi[j])
    m = spec.n_rows
    if bins is not None:
        bins = [int(bins)] * m if np.isscalar(bins) else [int(b) for b in bins]
        if len(bins) != m:
            raise ValueError("bins: one int or one per row")
        spec.bins[:m] = bins
    if centres is not None:
        if len(centres) != m:
            raise ValueError("centres: one per row")
        spec.centre[:m] = [float(c) for c in centres]
    if thresholds is not None:
        if isinstance(thresholds, dict):
            listed = list(spec.rows[:m])
            per_row = [[] for _ in range(m)]
            for r, values in thresholds.items():
                if _row_id(r) not in listed:
                    raise ValueError(f"thresholds: row {r!r} is not tallied")
                per_row[listed.index(_row_id(r))] = list(values)
        else:
            per_row = [list(t) for t in thresholds]
        if len(per_row) != m or any(len(t) > _abi.TALLY_MAX_THRESHOLDS for t in per_row):
            raise ValueError(f"thresholds: one list of at most {_abi.TALLY_MAX_THRESHOLDS} per row")
        for j, values in enumerate(per_row):
            spec.n_thresholds[j] = len(values)
            for t, v in enumerate(values):
                spec.threshold[j][t] = float(v)
    if k is not None:
        spec.k = int(k)
    if quantiles is not None:
        quantiles = [float(q) for q in quantiles]
        if len(quantiles) > _abi.TALLY_MAX_Q:
            raise ValueError(f"at most {_abi.TALLY_MAX_Q} quantiles")
        spec.n_q = len(quantiles)
        spec.q[:len(quantiles)] = quantiles
    for key, val in (bounds or {}).items():
        if key not in ("max_apogee", "min_apogee", "max_range", "max_flight_time", "energy_apogee"):
            raise ValueError(f"unknown bound {key!r}")
        setattr(spec, key, float(val))
    if grid_rows is not None:
        spec.row_x, spec.row_y = _row_id(grid_rows[0]), _row_id(grid_rows[1])
    if grid_bins is not None:
        spec.bins_x, spec.bins_y = (int(grid_bins),) * 2 if np.isscalar(grid_bins) else (int(grid_bins[0]), int(grid_bins[1]))
    if grid_ranges is not None:
        (spec.lo_x, spec.hi_x), (spec.lo_y, spec.hi_y) = [(float(lo), float(hi)) for lo, hi in grid_ranges]
    if zones is not None:
        zones = [np.asarray(z, dtype=np.float64).reshape(-1, 2) for z in zones]
        if len(zones) > _abi.TALLY_MAX_ZONES or sum(len(z) for z in zones) > _abi.TALLY_MAX_VERTICES:
            raise ValueError(f"at most {_abi.TALLY_MAX_ZONES} zones of {_abi.TALLY_MAX_VERTICES} vertices together")
        spec.n_zones, at = len(zones), 0
        for z, poly in enumerate(zones):
            spec.zone_first[z] = at
            spec.zone_x[at:at + len(poly)] = poly[:, 0].tolist()
            spec.zone_y[at:at + len(poly)] = poly[:, 1].tolist()
            at += len(poly)
        spec.zone_first[len(zones)] = at
    return spec


def tally_words(spec):
    """The size of a tally's state in int64 words (erpl_mc_tally_words: refuses a bad spec with the library's message)."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    words = C.c_int64()
    _abi.check(lib, lib.erpl_mc_tally_words(C.byref(spec), C.byref(words)), "erpl_mc_tally_words")
    return int(words.value)


def tally_edges(lo, hi, bins):
    """The bin edges of a tallied row or grid axis: those of erpl_mc_histogram (np.linspace's two roundings, the last edge
    exact)."""
    e = np.arange(bins + 1, dtype=np.float64) * np.float64((hi - lo) / bins) + np.float64(lo)
    e[bins] = hi
    return e


def tally_statistics(result, level=0.95):
    """A tally's result (the dict of TrajectoryEngine.tally_result or tally_result_host) in the shape of
    `device_statistics` where a counterpart exists - n_samples, n_outliers, per tallied row name {'mean', 'std', 'min',
    'max', 'percentiles'}, reason_counts, termination_counts, n_non_finite - plus, per row: 'count', 'below', 'above',
    'moment_skipped', 'percentiles_exact', 'histogram' {'edges', 'counts'}, 'exceedance' [{'threshold', 'count',
    'probability', 'interval'}] (probability = count / counted values of the row, Wilson score interval at `level`),
    'smallest' / 'largest' [(value, id)]; 'grid' {'counts', 'edges_x', 'edges_y', 'counted', 'outside'} and 'zones'
    [{'vertices', 'inside', 'probability', 'interval'}] (probability = inside / grid counted).  A pure host function."""
    from . import _abi
    spec, res = result["spec"], result["result"]
    m, nq = spec.n_rows, spec.n_q
    out = {"n": int(res.n), "n_samples": int(res.n_valid), "n_failed": 0, "n_outliers": int(res.n_outliers), "interval_level": float(level),
           "reason_counts": {name: int(res.reason_counts[b]) for b, name in enumerate(_abi.WHY_NAMES)},
           "termination_counts": {name: int(res.termination_counts[b]) for b, name in enumerate(_abi.END_NAMES)},
           "n_non_finite": int(res.n_status_nan), "q": list(spec.q[:nq]), "rows": {}}
    for j in range(m):
        r, row = spec.rows[j], res.row[j]
        count = int(row.count)
        d = {"row": int(r), "count": count, "below": int(row.below), "above": int(row.above), "moment_skipped": int(row.moment_skipped),
             "mean": row.mean, "std": row.std, "var": row.var, "min": row.min, "max": row.max, "centre": spec.centre[j],
             "sum_d": row.sum_d, "sum_d2": row.sum_d2,
             "percentiles": list(row.quantile[:nq]), "percentiles_exact": [bool(e) for e in row.quantile_exact[:nq]],
             "histogram": {"edges": tally_edges(spec.lo[j], spec.hi[j], spec.bins[j]),
                           "counts": result["hist_counts"][j, :spec.bins[j]].copy()},
             "exceedance": [{"threshold": spec.threshold[j][t], "count": int(row.exceed[t]),
                             "probability": int(row.exceed[t]) / count if count else float("nan"),
                             "interval": wilson_interval(int(row.exceed[t]), count, level)} for t in range(spec.n_thresholds[j])],
             "smallest": [(row.smallest[e].value, int(row.smallest[e].id)) for e in range(row.n_smallest)],
             "largest": [(row.largest[e].value, int(row.largest[e].id)) for e in range(row.n_largest)]}
        out["rows"][ROW_NAMES[r]] = d
        out[ROW_NAMES[r]] = {key: d[key] for key in ("mean", "std", "min", "max", "percentiles")}
    counted = int(res.grid_counted)
    out["grid"] = {"rows": (int(spec.row_x), int(spec.row_y)), "counts": result["grid_counts"],
                   "edges_x": tally_edges(spec.lo_x, spec.hi_x, spec.bins_x), "edges_y": tally_edges(spec.lo_y, spec.hi_y, spec.bins_y),
                   "counted": counted, "outside": int(res.grid_outside)}
    out["zones"] = []
    for z in range(spec.n_zones):
        v0, v1 = spec.zone_first[z], spec.zone_first[z + 1]
        inside = int(res.zone_inside[z])
        out["zones"].append({"vertices": np.column_stack([spec.zone_x[v0:v1], spec.zone_y[v0:v1]]), "inside": inside,
                             "probability": inside / counted if counted else float("nan"),
                             "interval": wilson_interval(inside, counted, level)})
    return out


def _tally_result_dict(spec, res, hist, grid):
    return {"spec": spec, "result": res, "hist_counts": hist, "grid_counts": grid.reshape(spec.bins_x, spec.bins_y)}


def tally_add_host(spec, state, summary, status=None, first_id=0):
    """erpl_mc_tally_add_host: folds the NumPy window summary ([16, n] float64, C order) / status ([n] int32 or None) into
    the NumPy int64 state, in place - the device's rule on host memory, the same bytes."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    summary = np.ascontiguousarray(summary, dtype=np.float64)
    if summary.ndim != 2 or summary.shape[0] != _abi.SUMMARY_DIM:
        raise ValueError(f"summary must be [{_abi.SUMMARY_DIM}, n]")
    n = summary.shape[1]
    if status is not None:
        status = np.ascontiguousarray(status, dtype=np.int32)
        if status.shape != (n,):
            raise ValueError("status must be [n]")
    if not (isinstance(state, np.ndarray) and state.dtype == np.int64 and state.flags.c_contiguous and state.size == tally_words(spec)):
        raise ValueError("state must be a contiguous int64 array of tally_words(spec) words")
    _abi.check(lib, lib.erpl_mc_tally_add_host(C.byref(spec), C.c_void_p(state.ctypes.data), C.c_void_p(summary.ctypes.data), max(n, 1),
                                               C.c_void_p(status.ctypes.data) if status is not None else None, n, int(first_id)),
               "erpl_mc_tally_add_host")
    return state


def tally_merge_host(spec, dst, src):
    """erpl_mc_tally_merge_host: dst += src, two NumPy int64 states of `spec`, in place."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    words = tally_words(spec)
    for s in (dst, src):
        if not (isinstance(s, np.ndarray) and s.dtype == np.int64 and s.flags.c_contiguous and s.size == words):
            raise ValueError("dst and src must be contiguous int64 arrays of tally_words(spec) words")
    _abi.check(lib, lib.erpl_mc_tally_merge_host(C.byref(spec), C.c_void_p(dst.ctypes.data), C.c_void_p(src.ctypes.data)),
               "erpl_mc_tally_merge_host")
    return dst


def tally_result_host(spec, state):
    """erpl_mc_tally_result_host of a NumPy int64 state: the dict `tally_statistics` takes ({'spec', 'result':
    _abi.ErplTally, 'hist_counts' int64 [8, 1024], 'grid_counts' int64 [bins_x, bins_y]})."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    state = np.ascontiguousarray(state, dtype=np.int64)
    if state.size != tally_words(spec):
        raise ValueError("state must hold tally_words(spec) words")
    res = _abi.ErplTally()
    hist = np.zeros((_abi.TALLY_MAX_ROWS, _abi.TALLY_MAX_BINS), dtype=np.int64)
    grid = np.zeros(spec.bins_x * spec.bins_y, dtype=np.int64)
    _abi.check(lib, lib.erpl_mc_tally_result_host(C.byref(spec), C.c_void_p(state.ctypes.data), C.byref(res), C.c_void_p(hist.ctypes.data),
                                                  C.c_void_p(grid.ctypes.data)), "erpl_mc_tally_result_host")
    return _tally_result_dict(spec, res, hist, grid)


# ---------------------------------------------------------------------------------- subset simulation: rare-event probabilities
def subset_spec(row="range", tail="upper", centre=None, bounds=None, seed=0, level=0, step=1):
    """The spec of erpl_mc_subset_limit_state / _propose (_abi.ErplSubsetSpec) on top of the library's defaults: g is the
    summary row `row` (ROW_NAMES or index) for tail='upper', minus it for 'lower'; with centre=(cx, cy) the miss distance of
    the impact point instead.  bounds: the dict of TrajectoryEngine.analyze.  A pure host function."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    spec = _abi.ErplSubsetSpec()
    _abi.check(lib, lib.erpl_mc_subset_defaults(C.byref(spec)), "erpl_mc_subset_defaults")
    if tail not in ("upper", "lower"):
        raise ValueError("tail: 'upper' or 'lower'")
    spec.row, spec.sign = _row_id(row), 1 if tail == "upper" else -1
    if centre is not None:
        spec.use_centre, spec.cx, spec.cy = 1, float(centre[0]), float(centre[1])
    for key, val in (bounds or {}).items():
        if key not in ("max_apogee", "min_apogee", "max_range", "max_flight_time", "energy_apogee"):
            raise ValueError(f"unknown bound {key!r}")
        setattr(spec, key, float(val))
    spec.seed, spec.level, spec.step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(level), int(step)
    return spec


def _np_ptr(a):
    import ctypes as C
    return None if a is None else C.c_void_p(a.ctypes.data)


def _np_matrix(a, dtype, what):
    """A NumPy matrix the _host calls may read or write in place: 1-D or 2-D, unit column stride.  Returns (rows, ld)."""
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.ndim in (1, 2) and (a.shape[-1] <= 1 or a.strides[-1] == a.itemsize)):
        raise ValueError(f"{what} must be a {np.dtype(dtype).name} NumPy array with unit column stride")
    if a.ndim == 1 or a.shape[0] == 1:
        return 1, max(int(a.shape[-1]), 1)
    if a.strides[0] % a.itemsize or a.strides[0] // a.itemsize < a.shape[1]:
        raise ValueError(f"{what}: rows must not overlap")
    return int(a.shape[0]), a.strides[0] // a.itemsize


def subset_limit_state_host(spec, summary, status=None):
    """erpl_mc_subset_limit_state_host: g [n] of the NumPy summary [16, n] / status [n] (or None)."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    summary = np.ascontiguousarray(summary, dtype=np.float64)
    n = summary.shape[1]
    status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
    g = np.empty(n, dtype=np.float64)
    _abi.check(lib, lib.erpl_mc_subset_limit_state_host(C.byref(spec), _np_ptr(summary), _np_ptr(status), n, n, _np_ptr(g)),
               "erpl_mc_subset_limit_state_host")
    return g


def subset_seeds_host(g, n_seeds, gathers=(), threshold=None):
    """erpl_mc_subset_seeds_host on NumPy arrays: the n_seeds samples of g that went furthest (ties to the lower id).  gathers:
    up to 4 (src, dst) pairs of matrices [rows, n] / [rows, >= n_seeds] (or vectors) of one dtype of 1, 4 or 8 bytes; the
    selected columns of src go, ascending in id, to columns 0 .. n_seeds - 1 of dst, in place.  Returns (idx int32 [n_seeds],
    selected uint8 [n], threshold, n_alive).  n_seeds = 0: the indicator of the given `threshold` and its count (as n_alive).
    A died-out level raises _abi.ErplError."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    g = np.ascontiguousarray(g, dtype=np.float64)
    n, n_seeds = g.size, int(n_seeds)
    idx, sel = np.empty(max(n_seeds, 0), dtype=np.int32), np.empty(n, dtype=np.uint8)
    thr, alive = C.c_double(0.0 if threshold is None else float(threshold)), C.c_int64(0)
    slots = (_abi.ErplSubsetGather * max(len(gathers), 1))()
    for q, (src, dst) in enumerate(gathers):
        rows, ld_src = _np_matrix(src, src.dtype, "a gather's src")
        rows_d, ld_dst = _np_matrix(dst, src.dtype, "a gather's dst")
        if rows_d != rows:
            raise ValueError("a gather's src and dst: the same rows")
        slots[q].src, slots[q].dst, slots[q].ld_src, slots[q].ld_dst = src.ctypes.data, dst.ctypes.data, ld_src, ld_dst
        slots[q].rows, slots[q].elem_size = rows, src.itemsize
    _abi.check(lib, lib.erpl_mc_subset_seeds_host(_np_ptr(g), n, n_seeds, _np_ptr(idx), _np_ptr(sel), C.byref(thr), C.byref(alive),
                                                  slots, len(gathers)), "erpl_mc_subset_seeds_host")
    return idx, sel, thr.value, int(alive.value)


def _subset_rows(kinds, rho, s, w):
    kinds = bytes(bytearray(int(k) for k in kinds))
    R = len(kinds)
    rho = np.ascontiguousarray(np.broadcast_to(np.asarray(rho, dtype=np.float64), (R,)))
    s = np.sqrt(1.0 - rho * rho) if s is None else np.ascontiguousarray(np.broadcast_to(np.asarray(s, dtype=np.float64), (R,)))
    w = s.copy() if w is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.float64), (R,)))
    return kinds, R, rho, s, w


def subset_propose_host(spec, kinds, rho, cur, first_chain=0, out=None, s=None, w=None):
    """erpl_mc_subset_propose_host: the candidates of the chains first_chain .. first_chain + count - 1 whose current states are
    the columns of the NumPy matrix cur [R, count] (unit column stride), for (spec.seed, spec.level, spec.step).  rho, s, w:
    scalars or one per row; s defaults to sqrt(1 - rho^2), w to s.  Returns out (new, or the given [R, >= count] matrix)."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    kinds, R, rho, s, w = _subset_rows(kinds, rho, s, w)
    rows, ld = _np_matrix(cur, np.float64, "cur")
    count = int(cur.shape[-1])
    if out is None:
        out = np.empty((R, count), dtype=np.float64)
    rows_o, ld_o = _np_matrix(out, np.float64, "out")
    if rows != R or rows_o != R:
        raise ValueError(f"cur and out must have {R} rows")
    _abi.check(lib, lib.erpl_mc_subset_propose_host(C.byref(spec), kinds, _np_ptr(rho), _np_ptr(s), _np_ptr(w), R, _np_ptr(cur), ld,
                                                    int(first_chain), count, _np_ptr(out), ld_o), "erpl_mc_subset_propose_host")
    return out


def subset_commit_host(threshold, g_cand, g_cur, g_next, triples=()):
    """erpl_mc_subset_commit_host on NumPy arrays, in place: g_next and the `next` of every (cand, cur, next) triple take the
    candidate's column where g_cand >= threshold and the current one otherwise.  Returns the number accepted."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    count = int(g_cand.shape[-1])
    for a in (g_cand, g_cur, g_next):
        _np_matrix(a, np.float64, "g_cand, g_cur and g_next")
    slots = (_abi.ErplSubsetTriple * max(len(triples), 1))()
    for q, (cand, cur, nxt) in enumerate(triples):
        rows, ld_cand = _np_matrix(cand, cand.dtype, "a triple's cand")
        rows_c, ld = _np_matrix(cur, cand.dtype, "a triple's cur")
        rows_n, ld_n = _np_matrix(nxt, cand.dtype, "a triple's next")
        if not (rows == rows_c == rows_n) or (rows > 1 and ld != ld_n):
            raise ValueError("a triple's cand, cur and next: the same rows, cur and next the same leading dimension")
        slots[q].cand, slots[q].cur, slots[q].next = cand.ctypes.data, cur.ctypes.data, nxt.ctypes.data
        slots[q].ld_cand, slots[q].ld, slots[q].rows, slots[q].elem_size = ld_cand, ld, rows, cand.itemsize
    thr, acc = C.c_double(float(threshold)), C.c_int64(0)
    _abi.check(lib, lib.erpl_mc_subset_commit_host(C.byref(thr), _np_ptr(g_cand), _np_ptr(g_cur), _np_ptr(g_next), slots, len(triples),
                                                   count, C.byref(acc)), "erpl_mc_subset_commit_host")
    return int(acc.value)


def subset_chain_stats_host(selected, chains, steps):
    """erpl_mc_subset_chain_stats_host: (n1, pair int64 [steps - 1]) of the step-major indicator bytes [steps * chains]."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    selected = np.ascontiguousarray(selected, dtype=np.uint8)
    if selected.size != int(chains) * int(steps):
        raise ValueError("selected must hold steps * chains bytes")
    n1, pair = C.c_int64(0), np.zeros(max(int(steps) - 1, 1), dtype=np.int64)
    _abi.check(lib, lib.erpl_mc_subset_chain_stats_host(_np_ptr(selected), int(chains), int(steps), C.byref(n1), _np_ptr(pair)),
               "erpl_mc_subset_chain_stats_host")
    return int(n1.value), pair[:int(steps) - 1]


def subset_delta(n1, pair, chains, steps, chained):
    """(p, delta, gamma) of a level from its chain statistics (Au & Beck 2001): p = n1 / N, R(k) = pair[k - 1] / (N - k C) - p^2,
    gamma = 2 sum_k (1 - k / T) R(k) / (p (1 - p)) (0 for chained=False, level 0), delta^2 = (1 - p) / (p N) (1 + gamma)."""
    C_, T = int(chains), int(steps)
    N = C_ * T
    p = n1 / N
    gamma = 0.0
    if chained and 0 < n1 < N and T > 1:
        k = np.arange(1, T, dtype=np.float64)
        Rk = np.asarray(pair, dtype=np.float64) / (N - k * C_) - p * p
        gamma = float(2.0 * np.sum((1.0 - k / T) * Rk) / (p * (1.0 - p)))
    delta2 = (1.0 - p) / (p * N) * (1.0 + gamma) if n1 > 0 else float("nan")
    return p, math.sqrt(max(delta2, 0.0)) if delta2 == delta2 else float("nan"), gamma


class _SubsetHost:
    """The steps of a level on NumPy arrays (the _host calls)."""
    def empty(self, rows, n, like):
        return np.empty((rows, n) if rows else (n,), dtype=like.dtype)

    def check(self, a, shape, dtype, what):
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and tuple(a.shape) == shape):
            raise ValueError(f"{what} must be a {np.dtype(dtype).name} NumPy array of shape {shape}")
        return np.ascontiguousarray(a)

    def seeds(self, g, n_seeds, gathers):
        _, sel, thr, alive = subset_seeds_host(g, n_seeds, gathers)
        return sel, thr, alive

    def alive(self, g):
        return int(np.count_nonzero(g > -np.inf))

    def indicator(self, g, threshold):
        return subset_seeds_host(g, 0, threshold=threshold)[1]

    def propose(self, spec, kinds, rho, s, w, cur, cand):
        subset_propose_host(spec, kinds, rho, cur, 0, cand, s, w)

    def begin_level(self, threshold):
        self.threshold, self.accepted = threshold, 0

    def commit(self, g_cand, g_cur, g_next, triples):
        self.accepted += subset_commit_host(self.threshold, g_cand, g_cur, g_next, triples)

    def chain_stats(self, sel, chains, steps):
        return subset_chain_stats_host(sel, chains, steps)

    def read_accepted(self):
        return self.accepted

    def numpy(self, a):
        return np.array(a, copy=True)


class _SubsetDevice:
    """The steps of a level on device tensors (TrajectoryEngine.subset_*); the accept count stays on the device for a level."""
    def __init__(self, engine):
        import torch
        self.eng, self.torch = engine, torch
        self.acc = torch.zeros(1, dtype=torch.int64, device=engine.device)

    def empty(self, rows, n, like):
        return self.torch.empty((rows, n) if rows else (n,), dtype=like.dtype, device=self.eng.device)

    def check(self, a, shape, dtype, what):
        tdt = {np.float64: self.torch.float64, np.int32: self.torch.int32}[dtype]
        if not (self.torch.is_tensor(a) and a.device == self.eng.device and a.dtype == tdt and tuple(a.shape) == shape):
            raise ValueError(f"{what} must be a {np.dtype(dtype).name} tensor of shape {shape} on {self.eng.device}")
        return a.contiguous()

    def seeds(self, g, n_seeds, gathers):
        _, sel, thr, alive = self.eng.subset_seeds(g, n_seeds, gathers)
        both = self.torch.stack([thr, alive.to(self.torch.float64)]).cpu()   # one wait for the two words (alive < 2^31: exact)
        return sel, float(both[0]), int(both[1])

    def alive(self, g):
        return int((g > -math.inf).sum())

    def indicator(self, g, threshold):
        thr = self.torch.tensor(float(threshold), dtype=self.torch.float64, device=self.eng.device)
        return self.eng.subset_seeds(g, 0, threshold=thr)[1]

    def propose(self, spec, kinds, rho, s, w, cur, cand):
        self.eng.subset_propose(spec, kinds, rho, cur, 0, cand, s, w)

    def begin_level(self, threshold):
        self.threshold = self.torch.tensor(float(threshold), dtype=self.torch.float64, device=self.eng.device)
        self.acc.zero_()

    def commit(self, g_cand, g_cur, g_next, triples):
        self.eng.subset_commit(self.threshold, g_cand, g_cur, g_next, triples, self.acc)

    def chain_stats(self, sel, chains, steps):
        n1, pair = self.eng.subset_chain_stats(sel, chains, steps)
        both = self.torch.cat([n1.view(1), pair]).cpu().numpy()
        return int(both[0]), both[1:]

    def read_accepted(self):
        return int(self.acc)

    def numpy(self, a):
        return a.cpu().numpy()


def _subset_level_rows(value, level, R, what):
    """rho or width of chain level `level` (1-based): a scalar, one value per level (the last one repeats) or [levels][R]."""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        return np.full(R, float(a))
    a = a[min(level - 1, a.shape[0] - 1)]
    if a.ndim == 0:
        return np.full(R, float(a))
    if a.shape != (R,):
        raise ValueError(f"{what}: a scalar, one value per level or [levels][{R}]")
    return np.ascontiguousarray(a)


def subset_simulation(evaluate, draws0, kinds, *, chains, steps, target=None, max_levels=12, rho=0.8, width=None, seed=0,
                      engine=None, interval_level=0.95, curve_points=256):
    """Subset simulation (Au & Beck 2001, with the conditional-sampling proposal of Papaioannou et al. 2015) of P(g > target)
    over ANY evaluator, through the five steps of erpl_mc_subset_*.

    evaluate(draws [R, c]) -> g [c], or (g, summary [16, c] or None, status int32 [c] or None); it is called once with the
    N = chains * steps columns of level 0 and then with `chains` candidates per round.  draws0: the float64 [R, N] primitives
    of level 0 under the independent law - a device tensor (the device calls of `engine`, default the shared one; evaluate
    gets and returns device tensors) or a NumPy array (the _host calls).  kinds: one _abi.DESIGN_NORMAL / DESIGN_UNIFORM per
    row.  A NaN g counts as -inf.

    Every level selects the `chains` samples that went furthest as seeds (their g's smallest is the level's threshold) and
    grows each into a chain of `steps` states by steps - 1 rounds of propose -> evaluate -> commit.  The run stops at the
    first level whose threshold reaches `target`: the last factor is the share of that level's population with g >= target.
    Otherwise it stops after max_levels thresholds (with a target: the last factor is the share in the population grown
    from the last threshold, and 'reached' is False; target=None: P is that of the last threshold).  rho: the correlation of
    the proposal on normal rows - a scalar, one value per level or [levels][R]; width: the step of the uniform rows, likewise,
    default sqrt(1 - rho^2).

    Returns a dict: 'probability', 'cov' (Au & Beck's sqrt(sum delta_l^2): it ignores the correlation between levels and runs
    low - 0.18 estimated against 0.20 observed at 1e-6), 'interval' (log-normal, at interval_level), 'reached', 'levels' (one
    dict per factor: 'threshold', 'p', 'delta', 'gamma', 'n1', and 'acceptance': the share of the candidates that the chains
    grown from this threshold accepted, None where none were grown), 'thresholds', 'curve' (float64 [m, 2]: x
    ascending and P(g >= x), stitched from all levels down to the last population's largest g), 'curve_cov' (per point the
    c.o.v. of the factors its level is conditioned on: the band of the curve, without the binomial part), 'population' ('draws',
    'summary', 'status', 'g', 'indicator': the last level's population, step-major; with a target the indicator marks
    the failure sample), 'level0' ('g', 'summary', 'status' as evaluate returned them for draws0), 'evaluations' (columns
    handed to evaluate: N + (steps - 1) * chains per further level) and 'samples' (populations held x N).
    'warnings': a list of texts, empty for a healthy run - a level whose chains accepted under 1 % of their candidates, or whose
    threshold does not exceed the one before: the chains do not move (a failure region that is an island in the space of the
    primitives is not reached by local steps), and then NEITHER the probability NOR its c.o.v. is to be trusted.
    A level with fewer than `chains` samples of g > -inf has died out: ValueError at level 0, before any proposal, and
    _abi.ErplError later."""
    from . import _abi
    from scipy.special import ndtri
    C_, T = int(chains), int(steps)
    if C_ < 1 or not 1 <= T <= _abi.SUBSET_MAX_STEPS:
        raise ValueError(f"chains >= 1 and 1 <= steps <= {_abi.SUBSET_MAX_STEPS}")
    N, max_levels = C_ * T, int(max_levels)
    if max_levels < 1:
        raise ValueError("max_levels >= 1")
    kinds = bytes(bytearray(int(k) for k in kinds))
    R = len(kinds)
    if isinstance(draws0, np.ndarray):
        be = _SubsetHost()
    else:
        if engine is None:
            from .simulator import shared_engine
            engine = shared_engine(draws0.device)
        be = _SubsetDevice(engine)
    pop = be.check(draws0, (R, N), np.float64, "draws0")

    def call(x, c):
        out = evaluate(x)
        g, summ, st = out if isinstance(out, tuple) else (out, None, None)
        g = be.check(g, (c,), np.float64, "g of evaluate")
        summ = None if summ is None else be.check(summ, (_abi.SUMMARY_DIM, c), np.float64, "summary of evaluate")
        st = None if st is None else be.check(st, (c,), np.int32, "status of evaluate")
        return g, summ, st

    g, summ, status = call(pop, N)
    level0 = {"g": g, "summary": summ, "status": status}
    evaluations, populations = N, 1
    alive0 = be.alive(g)
    if alive0 < C_:
        raise ValueError(f"level 0 holds {alive0} valid samples (g > -inf), fewer than chains = {C_}")
    nxt, g_nxt = be.empty(R, N, pop), be.empty(0, N, g)
    summ_nxt = None if summ is None else be.empty(_abi.SUMMARY_DIM, N, summ)
    status_nxt = None if status is None else be.empty(0, N, status)
    cand = be.empty(R, C_, pop)
    levels, curve, P, reached, sel = [], [], 1.0, False, None
    z = float(ndtri(0.5 + 0.5 * float(interval_level)))

    def factor(sel, threshold, chained):
        n1, pair = be.chain_stats(sel, C_, T)
        p, delta, gamma = subset_delta(n1, pair, C_, T, chained)
        levels.append({"threshold": float(threshold), "p": p, "delta": delta, "gamma": gamma, "acceptance": None, "n1": n1})
        return p

    def stitch(g_host, P_level, upto):
        """The points of this level's population below `upto` (None: all): x ascending, P(g >= x) = P_level * share."""
        x = np.sort(g_host[g_host > -np.inf])
        share = (x.size - np.arange(x.size)) / N
        keep = np.ones(x.size, dtype=bool) if upto is None else x < upto
        x, share = x[keep], share[keep]
        if x.size > curve_points:
            pick = np.unique(np.linspace(0, x.size - 1, curve_points).round().astype(np.int64))
            x, share = x[pick], share[pick]
        before = math.sqrt(sum(lv["delta"] ** 2 for lv in levels))      # of the factors that condition this level
        curve.append(np.column_stack([x, P_level * share, np.full(x.size, before)]))

    for level in range(max_levels + 1):
        if level == max_levels:   # no threshold reached the target (or none was asked for): the population of the last one
            if target is not None:
                sel = be.indicator(g, target)
                P_before = P
                P *= factor(sel, target, True)
                stitch(be.numpy(g), P_before, None)
            else:
                sel = be.indicator(g, -math.inf)
                stitch(be.numpy(g), P, None)
            break
        gathers = [(pop, nxt), (g, g_nxt)]
        if summ is not None:
            gathers.append((summ, summ_nxt))
        if status is not None:
            gathers.append((status, status_nxt))
        sel, thr, alive = be.seeds(g, C_, gathers)
        if alive < C_:
            raise _abi.ErplError(f"subset simulation: level {level} has died out ({alive} samples with g > -inf, {C_} seeds needed)")
        if target is not None and thr >= target:
            sel = be.indicator(g, target)
            P_before = P
            P *= factor(sel, target, level > 0)
            stitch(be.numpy(g), P_before, None)
            reached = True
            break
        stitch(be.numpy(g), P, thr)
        P *= factor(sel, thr, level > 0)
        rho_l = _subset_level_rows(rho, level + 1, R, "rho")
        s_l = np.sqrt(1.0 - rho_l * rho_l)
        w_l = s_l if width is None else _subset_level_rows(width, level + 1, R, "width")
        be.begin_level(thr)
        spec = subset_spec(seed=seed, level=level + 1)
        for t in range(1, T):
            spec.step = t
            a, b = (t - 1) * C_, t * C_
            be.propose(spec, kinds, rho_l, s_l, w_l, nxt[:, a:b], cand)
            gc, sc, stc = call(cand, C_)
            evaluations += C_
            triples = [(cand, nxt[:, a:b], nxt[:, b:b + C_])]
            if summ is not None:
                triples.append((sc, summ_nxt[:, a:b], summ_nxt[:, b:b + C_]))
            if status is not None:
                triples.append((stc, status_nxt[a:b], status_nxt[b:b + C_]))
            be.commit(gc, g_nxt[a:b], g_nxt[b:b + C_], triples)
        levels[-1]["acceptance"] = be.read_accepted() / (C_ * (T - 1)) if T > 1 else None
        if level == 0:   # level 0 is the caller's (draws0) and the result's ('level0'): the chains never write into it
            pop, g, summ, status = be.empty(R, N, pop), be.empty(0, N, g), None if summ is None else be.empty(_abi.SUMMARY_DIM, N, summ), \
                None if status is None else be.empty(0, N, status)
        pop, nxt, g, g_nxt = nxt, pop, g_nxt, g
        summ, summ_nxt, status, status_nxt = summ_nxt, summ, status_nxt, status
        populations += 1
    # What the estimate cannot see by itself: chains that do not move.  A failure region that is an island in the space of
    # the primitives (a second mode the bulk does not lead to) is not reached by local steps; the levels then slice one frozen
    # sample ever thinner, P falls by p0 per level and delta stays small.
    warnings = []
    for l, lv in enumerate(levels):
        if lv["acceptance"] is not None and lv["acceptance"] < 0.01:
            warnings.append(f"level {l}: the chains grown from the threshold {lv['threshold']:.6g} accepted {lv['acceptance']:.2g} of "
                            "their candidates - they do not move; the probability and its c.o.v. are not to be trusted "
                            "(a larger rho takes smaller steps; a failure mode the bulk does not lead to needs direct sampling)")
        if 0 < l < len(levels) - (1 if target is not None else 0) and lv["threshold"] <= levels[l - 1]["threshold"]:
            warnings.append(f"level {l}: the threshold {lv['threshold']:.6g} does not exceed the one before - the seeds are copies")
    cov = math.sqrt(sum(lv["delta"] ** 2 for lv in levels)) if levels else 0.0
    sigma = math.sqrt(math.log1p(cov * cov)) if cov == cov else float("nan")
    return {"probability": P, "cov": cov, "interval": (P * math.exp(-z * sigma), P * math.exp(z * sigma)),
            "interval_level": float(interval_level), "reached": reached, "target": target, "levels": levels,
            "thresholds": [lv["threshold"] for lv in levels], "curve": np.concatenate(curve)[:, :2], "curve_cov": np.concatenate(curve)[:, 2],
            "population": {"draws": pop, "summary": summ, "status": status, "g": g, "indicator": sel}, "level0": level0,
            "chains": C_, "steps": T, "evaluations": evaluations, "samples": populations * N, "warnings": warnings}


# ---------------------------------------------------------------------------------- reweighting: a flown run under another law
def reweight_spec(kinds, law, rows=None, thresholds=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95)):
    """The spec of erpl_mc_reweight (_abi.ErplRwSpec) on top of the library's defaults.  kinds: per law row
    _abi.DESIGN_NORMAL or _abi.DESIGN_UNIFORM; law: per law row the target, (mu, s) in flown sigmas for a normal row and
    (a, b) within the flown (0, 1) for a uniform row.  rows: up to 4 summary rows (ROW_NAMES or index, _abi.RW_ROW_EXTRA for
    `extra`; default apogee, range, flight time); thresholds: None or a mapping row -> up to 8 thresholds (keys as in
    `rows`); quantiles: up to 8.  A pure host function; the values are checked by the library."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    spec = _abi.ErplRwSpec()
    _abi.check(lib, lib.erpl_mc_reweight_defaults(C.byref(spec)), "erpl_mc_reweight_defaults")
    kinds = [int(k) for k in kinds]
    law = [tuple(float(v) for v in p) for p in law]
    if len(kinds) != len(law) or not 1 <= len(kinds) <= _abi.RW_MAX_LAW or any(len(p) != 2 for p in law):
        raise ValueError(f"kinds and law: one entry per law row, 1 to {_abi.RW_MAX_LAW} of them, law entries (mu, s) or (a, b)")
    spec.n_law = len(kinds)
    for r, (k, p) in enumerate(zip(kinds, law)):
        spec.kind[r] = k & 0xFF
        if k == _abi.DESIGN_NORMAL:
            spec.mu[r], spec.s[r] = p
        else:
            spec.a[r], spec.b[r] = p
    if rows is not None:
        ids = [_abi.RW_ROW_EXTRA if r == "extra" else _row_id(r) for r in rows]
        if not 1 <= len(ids) <= _abi.RW_MAX_ROWS:
            raise ValueError(f"1 to {_abi.RW_MAX_ROWS} rows")
        spec.n_rows = len(ids)
        spec.rows[:len(ids)] = ids
    have = list(spec.rows[:spec.n_rows])
    for key, values in (thresholds or {}).items():
        r = _abi.RW_ROW_EXTRA if key == "extra" else _row_id(key)
        if r not in have:
            raise ValueError(f"thresholds: row {key!r} is not among the requested rows")
        values = [float(v) for v in values]
        if len(values) > _abi.RW_MAX_THRESHOLDS:
            raise ValueError(f"at most {_abi.RW_MAX_THRESHOLDS} thresholds per row")
        j = have.index(r)
        spec.n_thresholds[j] = len(values)
        spec.threshold[j][:len(values)] = values
    quantiles = [float(q) for q in quantiles]
    if len(quantiles) > _abi.RW_MAX_Q:
        raise ValueError(f"at most {_abi.RW_MAX_Q} quantiles")
    spec.n_q = len(quantiles)
    spec.q[:len(quantiles)] = quantiles
    return spec


def reweight_result_dict(spec, res):
    """An _abi.ErplReweight as a plain dict: the counts, Q, sum_w, max_w (Python ints), sum_w2, ess, ess_expected_share and
    'rows': per requested row id its mean, mean_se, var, std, min, max, q / quantiles and thresholds / exceed_w / p / p_se."""
    out = {k: int(getattr(res, k)) for k in ("n", "count", "n_masked", "n_non_finite", "n_outside", "n_zero", "Q", "sum_w", "max_w")}
    out.update(sum_w2=res.sum_w2, ess=res.ess, ess_expected_share=res.ess_expected_share)
    nq = spec.n_q
    out["rows"] = {}
    for j in range(spec.n_rows):
        r, nt = res.row[j], spec.n_thresholds[j]
        out["rows"][int(spec.rows[j])] = {
            "mean": r.mean, "mean_se": r.mean_se, "var": r.var, "std": r.std, "min": r.min, "max": r.max,
            "q": list(spec.q[:nq]), "quantiles": list(r.quantile[:nq]), "thresholds": list(spec.threshold[j][:nt]),
            "exceed_w": [int(v) for v in r.exceed_w[:nt]], "p": list(r.p[:nt]), "p_se": list(r.p_se[:nt])}
    return out


def reweight_host(factors, kinds, law, summary, mask=None, rows=None, extra=None, thresholds=None,
                  quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), want_weights=False):
    """erpl_mc_reweight_host on NumPy arrays - TrajectoryEngine.reweight without a device, the same integers and the same
    log-weights: factors float64 [n_law, n] (unit column stride), summary float64 [16, n] (likewise), mask uint8 [n] or None,
    extra float64 [n] or None.  Returns the dict of `reweight_result_dict`; want_weights adds 'logw' (float64 [n]) and
    'weights' (int64 [n])."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    spec = reweight_spec(kinds, law, rows, thresholds, quantiles)
    n_law, ld = _np_matrix(factors, np.float64, "factors")
    n = int(factors.shape[-1])
    s_rows, ld_s = _np_matrix(summary, np.float64, "summary")
    if n_law != spec.n_law or s_rows != _abi.SUMMARY_DIM or summary.shape[1] != n:
        raise ValueError(f"factors must be [{spec.n_law}, n] and summary [{_abi.SUMMARY_DIM}, n]")
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if mask.shape != (n,):
            raise ValueError("mask must be [n]")
    if extra is not None:
        extra = np.ascontiguousarray(extra, dtype=np.float64)
        if extra.shape != (n,):
            raise ValueError("extra must be [n]")
    logw = np.empty(n, dtype=np.float64) if want_weights else None
    weights = np.empty(n, dtype=np.int64) if want_weights else None
    res = _abi.ErplReweight()
    _abi.check(lib, lib.erpl_mc_reweight_host(C.byref(spec), _np_ptr(factors), ld, _np_ptr(summary), ld_s, _np_ptr(extra), _np_ptr(mask), n,
                                              C.byref(res), _np_ptr(logw), _np_ptr(weights)), "erpl_mc_reweight_host")
    out = reweight_result_dict(spec, res)
    if want_weights:
        out["logw"], out["weights"] = logw, weights
    return out


def finish_reweighted(out):
    """What `reweighted_statistics` adds to the dict of TrajectoryEngine.reweight that needs no device (in place): 'ess_share'
    = ess / (count + n_outside) - the share of the FLOWN samples, those outside the target's support included, which is what
    ess_expected_share is the expectation of - 'max_weight_share' = max_w / sum_w, 'row_names', and 'warnings' - an infinite weight variance
    (ess_expected_share == 0: a normal row widened to s^2 >= 2), ess < 100, max_weight_share > 0.1, an empty support."""
    from . import _abi
    empty = out["count"] == 0 or out["sum_w"] == 0
    out["ess_share"] = math.nan if empty else out["ess"] / (out["count"] + out["n_outside"])
    out["max_weight_share"] = math.nan if empty else out["max_w"] / out["sum_w"]
    out["row_names"] = ["extra" if r == _abi.RW_ROW_EXTRA else ROW_NAMES[r] for r in out["rows"]]
    warnings = []
    if out["ess_expected_share"] == 0.0:
        warnings.append("the variance of the weights is infinite (a normal row is widened to s^2 >= 2): no error bar holds")
    if empty:
        warnings.append("the support is empty: no flown sample lies inside the target law")
    else:
        if out["ess"] < 100.0:
            warnings.append(f"the effective sample size is {out['ess']:.1f}, below 100: fly a new run")
        if out["max_weight_share"] > 0.1:
            warnings.append(f"one sample carries {100.0 * out['max_weight_share']:.1f} % of the weight")
    out["warnings"] = warnings
    return out


def reweighted_statistics(summary, factors, kinds, law, status=None, engine=None, rows=None, extra=None, thresholds=None,
                          quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), want_weights=False):
    """The statistics of a flown run of INDEPENDENT primitives (a run flown with design=...) under another input law, without
    a new run: erpl_mc_analyze for the reason bytes (as `drivers`), then erpl_mc_reweight (TrajectoryEngine.reweight) of
    the changed primitive rows `factors` (float64 [n_law, n] device tensor; `kinds`, `law` as in `reweight_spec`) over the
    samples the filter keeps.  Returns the dict of TrajectoryEngine.reweight - per row mean +- mean_se, std, quantiles and
    the exceedance probabilities p +- p_se - plus 'n_samples', 'n_outliers' and what `finish_reweighted` adds: ess_share,
    max_weight_share, row_names and warnings.

    Reading it: the error bars are the delta method for a ratio of sums over i.i.d. columns - conservative for an 'lhs' or
    'qmc' run.  Trust the answer as far as ess goes: narrowing a law works, widening one does not (the heaviest tail
    samples take the weight), and ess_share is a product over the changed rows, so changing many at once costs
    exponentially."""
    engine, res, why = _filter(summary, status, engine)
    out = engine.reweight(factors, kinds, law, summary, mask=why, rows=rows, extra=extra, thresholds=thresholds, quantiles=quantiles,
                          want_weights=want_weights)
    out["n_samples"], out["n_outliers"] = int(res.n_valid), int(res.n_outliers)
    return finish_reweighted(out)


def reweighted_impact(summary, factors, kinds, law, status=None, engine=None, target=None, cep_quantiles=(0.5, 0.9, 0.95),
                      **density_kw):
    """The impact probability map of a flown run of INDEPENDENT primitives under another input law, without a new run, in
    three steps on the device: erpl_mc_analyze for the reason bytes (as `reweighted_statistics`); erpl_mc_reweight with
    want_weights over the one row `extra` = the miss distance about `target` ((x, y), default the launch site at the
    origin); erpl_mc_impact_density_weighted (TrajectoryEngine.impact_density_weighted, `density_kw` are its keywords:
    nodes, ranges, pad, bandwidth, levels, zones, sample_density, rows) with those weights.  Returns the map's dict plus
    'cep' ({'q', 'quantiles', 'mean', 'mean_se'}: the weighted quantiles of the miss distance), per zone 'probability' =
    weight / sum_w with 'se' by the formula of erpl_mc_reweight's p_se and 'interval' = probability -+ 1.96 se within
    [0, 1], 'n_samples' / 'n_outliers' of the filter, and of the reweighting: Q, n_outside, ess_expected_share and what
    `finish_reweighted` adds - ess_share, max_weight_share, warnings.  ('ess' is the map's: over the samples that have an
    impact point.)  Read it as `reweighted_statistics` says: trust the map as far as ess goes."""
    import torch
    from . import _abi
    engine, res, why = _filter(summary, status, engine)
    rows = density_kw.get("rows", (_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y))
    tx, ty = (0.0, 0.0) if target is None else (float(target[0]), float(target[1]))
    miss = torch.hypot(summary[int(rows[0])] - tx, summary[int(rows[1])] - ty).contiguous()
    rw = engine.reweight(factors, kinds, law, summary, mask=why, rows=[_abi.RW_ROW_EXTRA], extra=miss,
                         quantiles=cep_quantiles, want_weights=True)
    out = engine.impact_density_weighted(summary, rw["weights"], why, **density_kw)
    out["n_samples"], out["n_outliers"] = int(res.n_valid), int(res.n_outliers)
    r = rw["rows"][_abi.RW_ROW_EXTRA]
    out["target"] = (tx, ty)
    out["cep"] = {"q": r["q"], "quantiles": r["quantiles"], "mean": r["mean"], "mean_se": r["mean_se"]}
    s_d = math.ldexp(float(out["sum_w"]), -out["max_w"].bit_length())   # sum_w2 and a2 are in weights scaled alike
    for z in out["zones"]:
        if out["sum_w"] == 0:
            z["probability"], z["se"], z["interval"] = math.nan, math.nan, (0.0, 1.0)
            continue
        prob = z["weight"] / out["sum_w"]
        z["probability"] = prob
        z["se"] = math.sqrt(max((1.0 - 2.0 * prob) * z["a2"] + prob * prob * out["sum_w2"], 0.0)) / s_d
        z["interval"] = (max(0.0, prob - 1.96 * z["se"]), min(1.0, prob + 1.96 * z["se"]))
    fin = finish_reweighted(rw)
    for k in ("Q", "n_outside", "ess_expected_share", "ess_share", "max_weight_share", "warnings"):
        out[k] = fin[k]
    return out


def bands_weighted_spec(n_channels, n_nodes, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), thresholds=None):
    """The spec of erpl_mc_corridor_bands_weighted (_abi.ErplBandsWSpec) on top of the library's defaults.  quantiles: up to
    8; thresholds: None, or per channel (a sequence of n_channels entries, or a mapping channel index -> entry) up to 4
    thresholds.  A pure host function; the values are checked by the library."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    spec = _abi.ErplBandsWSpec()
    _abi.check(lib, lib.erpl_mc_corridor_bands_weighted_defaults(C.byref(spec)), "erpl_mc_corridor_bands_weighted_defaults")
    n_channels, n_nodes = int(n_channels), int(n_nodes)
    if not 1 <= n_channels <= _abi.CORRIDOR_MAX_CHANNELS:
        raise ValueError(f"1 to {_abi.CORRIDOR_MAX_CHANNELS} channels")
    if not 1 <= n_nodes <= _abi.CORRIDOR_MAX_NODES:
        raise ValueError(f"1 to {_abi.CORRIDOR_MAX_NODES} nodes")
    spec.n_channels, spec.n_nodes = n_channels, n_nodes
    quantiles = [float(q) for q in quantiles]
    if len(quantiles) > _abi.RW_MAX_Q:
        raise ValueError(f"at most {_abi.RW_MAX_Q} quantiles")
    spec.n_q = len(quantiles)
    spec.q[:len(quantiles)] = quantiles
    if thresholds is not None:
        items = thresholds.items() if hasattr(thresholds, "items") else enumerate(thresholds)
        for c, values in items:
            c = int(c)
            if not 0 <= c < n_channels:
                raise ValueError(f"thresholds: channel {c} outside 0..{n_channels - 1}")
            values = [] if values is None else [float(v) for v in values]
            if len(values) > _abi.BANDS_W_MAX_THRESHOLDS:
                raise ValueError(f"at most {_abi.BANDS_W_MAX_THRESHOLDS} thresholds per channel")
            spec.n_thresholds[c] = len(values)
            spec.threshold[c][:len(values)] = values
    return spec


def bands_weighted_result_dict(spec, rows, res):
    """The records of erpl_mc_corridor_bands_weighted as a dict of NumPy arrays: 'count', 'n_non_finite', 'n_zero', 'sum_w'
    int64 [C, T]; 'min', 'max', 'mean', 'var', 'std', 'mean_se', 'sum_w2', 'ess' float64 [C, T]; 'quantiles' float64
    [C, n_q, T]; 'exceed_w' int64, 'a2', 'p', 'p_se' float64 [C, 4, T] (entries past a channel's thresholds: 0 / NaN; p and
    p_se by erpl_mc_reweight's formula); 'q', 'thresholds' (per channel a list) and Python ints 'm', 'n_masked', 'n_counted',
    'max_w', 'K', 'Q'."""
    from . import _abi
    Cn, T, nq, nt = spec.n_channels, spec.n_nodes, spec.n_q, _abi.BANDS_W_MAX_THRESHOLDS
    words = 12 + _abi.RW_MAX_Q + 2 * nt   # erpl_bands_w_row in eight-byte words
    ints = np.frombuffer(rows, dtype=np.int64).reshape(Cn, T, words)
    raw = np.frombuffer(rows, dtype=np.float64).reshape(Cn, T, words)
    out = {name: ints[:, :, k].copy() for k, name in enumerate(("count", "n_non_finite", "n_zero", "sum_w"))}
    out["exceed_w"] = np.ascontiguousarray(ints[:, :, 4:4 + nt].transpose(0, 2, 1))
    at = 4 + nt
    out["quantiles"] = np.ascontiguousarray(raw[:, :, at:at + nq].transpose(0, 2, 1))
    at += _abi.RW_MAX_Q
    for k, name in enumerate(("min", "max", "mean", "var", "std", "mean_se", "sum_w2", "ess")):
        out[name] = raw[:, :, at + k].copy()
    out["a2"] = np.ascontiguousarray(raw[:, :, at + 8:at + 8 + nt].transpose(0, 2, 1))
    K = int(res.K)
    with np.errstate(invalid="ignore", divide="ignore"):
        s_d = np.ldexp(out["sum_w"].astype(np.float64), -K)[:, None, :]
        p = out["exceed_w"].astype(np.float64) / out["sum_w"].astype(np.float64)[:, None, :]
        v = (1.0 - 2.0 * p) * out["a2"] + (p * p) * out["sum_w2"][:, None, :]
        out["p"], out["p_se"] = p, np.sqrt(np.maximum(v, 0.0)) / s_d
    for c in range(Cn):
        out["p"][c, spec.n_thresholds[c]:], out["p_se"][c, spec.n_thresholds[c]:] = np.nan, np.nan
    out["q"] = list(spec.q[:nq])
    out["thresholds"] = [list(spec.threshold[c][:spec.n_thresholds[c]]) for c in range(Cn)]
    out.update({k: int(getattr(res, k)) for k in ("m", "n_masked", "n_counted", "max_w", "K", "Q")})
    return out


def bands_weighted_host(values, weights, mask=None, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), thresholds=None, m=None):
    """erpl_mc_corridor_bands_weighted_host on NumPy arrays - TrajectoryEngine.corridor_bands_weighted without a device, the
    same integers and the same order statistics: values float64 [C, T, ld] (C-contiguous) of which the first m columns are
    read (default ld), weights int64 [m], mask uint8 [m] or None.  Returns the dict of `bands_weighted_result_dict`."""
    import ctypes as C
    from . import _abi
    lib = _abi.load_library()
    if not (isinstance(values, np.ndarray) and values.dtype == np.float64 and values.ndim == 3 and values.flags.c_contiguous):
        raise ValueError("values must be a C-contiguous float64 [C, T, ld] array")
    Cn, T, ld = (int(s) for s in values.shape)
    m = ld if m is None else int(m)
    if not 1 <= m <= ld:
        raise ValueError(f"m = {m} outside 1..{ld}")
    spec = bands_weighted_spec(Cn, T, quantiles, thresholds)
    weights = np.ascontiguousarray(weights, dtype=np.int64)
    if weights.shape != (m,):
        raise ValueError("weights must be int64 [m]")
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if mask.shape != (m,):
            raise ValueError("mask must be uint8 [m]")
    rows = (_abi.ErplBandsWRow * (Cn * T))()
    res = _abi.ErplBandsWResult()
    _abi.check(lib, lib.erpl_mc_corridor_bands_weighted_host(_np_ptr(values), _np_ptr(mask), _np_ptr(weights), m, ld, C.byref(spec),
                                                             C.cast(rows, C.c_void_p), C.byref(res)),
               "erpl_mc_corridor_bands_weighted_host")
    return bands_weighted_result_dict(spec, rows, res)


def reweighted_corridor(values, t0, step, channels, factors, kinds, law, mask=None, engine=None,
                        quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), thresholds=None, m=None):
    """The time-resolved bands of a captured matrix (float64 [C, T, ld] on the device: a corridor, an impact-point or a debris
    matrix flown from a design of INDEPENDENT primitives) under another input law, without a new run.  ONE erpl_mc_reweight
    call gives the weights: the changed primitive rows `factors` (float64 [n_law, m] device tensor; `kinds`, `law` as in
    `reweight_spec`) over the columns whose `mask` byte is 0, with a row of zeros as the one requested row - so the weight
    population is the mask and the support of the target alone, whatever the matrix holds.  Then
    erpl_mc_corridor_bands_weighted describes every row over ITS OWN population under those weights, and
    erpl_mc_corridor_bands describes the same matrix as flown, for comparison.  `channels`: the names of the C channels; nodes
    at t0 + k step; m: the columns read (default: the columns of `factors`).
    Returns a dict: 'time' [T], 'channels', 'q', 'thresholds', per channel name 'reweighted' ({'count', 'mean', 'mean_se',
    'std', 'min', 'max', 'ess', 'sum_w' [T], 'quantiles' [n_q, T], 'p', 'p_se', 'exceed_w' [n_thr, T]}) and 'flown' (the
    unweighted {'count', 'mean', 'std', 'min', 'max', 'quantiles'}), the call record ('m', 'n_masked', 'n_counted', 'max_w',
    'K', 'Q') and of the reweighting 'count' (the columns the mask keeps inside the target's support), 'n_zero' (those of them
    whose weight rounds to 0), 'n_outside', 'sum_w', 'ess', 'ess_expected_share', 'ess_share', 'max_weight_share' and 'warnings'
    (`finish_reweighted`, plus the nodes whose own effective sample size is below 100).

    Reading it: the weighted quantile is the inverted-cdf order statistic, a flown value, not the interpolated one of the
    flown bands; mean_se is the delta-method error of a ratio of sums over i.i.d. columns.  Per node, `ess` says where not
    to believe the band: late nodes hold fewer flights, and a few heavy ones may carry them."""
    import torch
    from . import _abi
    engine = _engine_of(values, engine)
    if values.dim() != 3:
        raise ValueError("values must be a [C, T, ld] matrix")
    n_ch, n_nodes, ld = (int(s) for s in values.shape)
    channels = [CORRIDOR_CHANNEL_NAMES[c] if not isinstance(c, str) else c for c in channels]
    if len(channels) != n_ch:
        raise ValueError(f"{len(channels)} channels for a matrix of {n_ch}")
    m = int(factors.shape[-1]) if m is None else int(m)
    if not 1 <= m <= ld:
        raise ValueError(f"m = {m} outside 1..{ld}")
    zeros = torch.zeros(m, dtype=torch.float64, device=values.device)
    summary = torch.zeros((_abi.SUMMARY_DIM, m), dtype=torch.float64, device=values.device)   # no summary row is requested
    rw = engine.reweight(factors, kinds, law, summary, mask=mask, rows=[_abi.RW_ROW_EXTRA], extra=zeros, quantiles=(),
                         want_weights=True)
    w = engine.corridor_bands_weighted(values, rw["weights"], mask=mask, quantiles=quantiles, thresholds=thresholds, m=m)
    b = engine.corridor_bands(values, mask, quantiles=quantiles, m=m)
    fin = finish_reweighted(rw)
    out = {"time": float(t0) + np.arange(n_nodes, dtype=np.float64) * float(step), "channels": channels, "q": w["q"],
           "thresholds": w["thresholds"]}
    out.update({k: w[k] for k in ("m", "n_masked", "n_counted", "max_w", "K", "Q")})
    out.update({k: fin[k] for k in ("count", "n_zero", "n_outside", "sum_w", "ess", "ess_expected_share", "ess_share",
                                    "max_weight_share")})
    warnings = list(fin["warnings"])
    for c, name in enumerate(channels):
        nt = len(w["thresholds"][c])
        rew = {k: w[k][c] for k in ("count", "mean", "mean_se", "std", "min", "max", "ess", "sum_w", "quantiles")}
        rew.update({k: w[k][c][:nt] for k in ("p", "p_se", "exceed_w")})
        out[name] = {"reweighted": rew, "flown": {k: b[k][c] for k in ("count", "mean", "std", "min", "max", "quantiles")}}
        thin = np.flatnonzero((rew["count"] > 0) & (rew["ess"] < 100.0))
        if len(thin):
            warnings.append(f"{name}: the effective sample size is below 100 at {len(thin)} of {n_nodes} nodes "
                            f"(from node {int(thin[0])})")
    out["warnings"] = warnings
    return out


# ---------------------------------------------------------------------------------- the casualty expectation of a footprint
CASUALTY_COUNTS = ("landed", "lethal", "off_grid", "missing")   # rows 1..4 of per_node / per_fragment (_abi.CASUALTY_*)


def failure_probabilities(times, rate, t_end=None):
    """The probability that a launched vehicle breaks up in the interval every node stands for: p_k = exp(-L(t_k)) -
    exp(-L(t_k+1)) with L the integral of the failure rate (1/s) from 0.  times: the node times, ascending, >= 0; rate: a
    constant, or one value per node that holds from its node to the next (and from 0 to the first node).  The last node
    takes the interval to the end of the rate table, t_end: by default one more interval of the length of the one before
    it (a single node needs t_end).  Returns float64 [len(times)]; the values sum to at most 1."""
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    if len(t) < 1 or not np.isfinite(t).all() or t[0] < 0.0 or (np.diff(t) <= 0.0).any():
        raise ValueError("times: at least one finite value, not negative, ascending")
    if t_end is None:
        if len(t) < 2:
            raise ValueError("a single node needs t_end")
        t_end = t[-1] + (t[-1] - t[-2])
    t_end = float(t_end)
    if not (np.isfinite(t_end) and t_end > t[-1]):
        raise ValueError("t_end must lie behind the last node")
    r = np.asarray(rate, dtype=np.float64)
    r = np.full(len(t), float(r)) if r.ndim == 0 else r.reshape(-1)
    if len(r) != len(t) or not np.isfinite(r).all() or (r < 0.0).any():
        raise ValueError("rate: a constant or one value per node, finite and not negative")
    knots = np.append(t, t_end)
    L = r[0] * t[0] + np.concatenate(([0.0], np.cumsum(r * np.diff(knots))))   # L at every knot
    return np.exp(-L[:-1]) - np.exp(-L[1:])


def casualty_spec(n_nodes, fragments, bins, ranges, ke_min=15.0, smooth=True, bw_scale=1.0, h_floor=1.0, levels=(1e-6, 1e-5)):
    """The spec of erpl_mc_casualty (_abi.ErplCasualtySpec) on top of the library's defaults, every argument checked as a
    Python int or float before a 32-bit field can truncate it.  fragments: (pieces, area, mass) triples; bins: (bins_x,
    bins_y); ranges: ((lo_x, hi_x), (lo_y, hi_y))."""
    import ctypes as C
    from . import _abi
    n_nodes = int(n_nodes)
    frags = [tuple(float(v) for v in f) for f in fragments]
    if not 1 <= len(frags) <= _abi.DEBRIS_MAX_FRAGMENTS or any(len(f) != 3 for f in frags):
        raise ValueError(f"1 to {_abi.DEBRIS_MAX_FRAGMENTS} fragments, each (pieces, area, mass)")
    if not 1 <= n_nodes <= _abi.IIP_MAX_NODES or n_nodes * len(frags) > _abi.CORRIDOR_MAX_NODES:
        raise ValueError(f"1 to {_abi.IIP_MAX_NODES} nodes, at most {_abi.CORRIDOR_MAX_NODES} nodes * fragments")
    for f in frags:
        if not all(np.isfinite(v) and v >= 0.0 for v in f):
            raise ValueError("pieces, area and mass of a fragment must be finite and not negative")
    bins_x, bins_y = (int(b) for b in bins)
    if not (1 <= bins_x <= _abi.CASUALTY_MAX_GRID and 1 <= bins_y <= _abi.CASUALTY_MAX_GRID):
        raise ValueError(f"1 to {_abi.CASUALTY_MAX_GRID} cells per axis")
    (lo_x, hi_x), (lo_y, hi_y) = ((float(a), float(b)) for a, b in ranges)
    if not (np.isfinite([lo_x, hi_x, lo_y, hi_y]).all() and lo_x < hi_x and lo_y < hi_y):
        raise ValueError("ranges: ((lo_x, hi_x), (lo_y, hi_y)), finite, lo < hi")
    ke_min, bw_scale, h_floor = float(ke_min), float(bw_scale), float(h_floor)
    if not (np.isfinite(ke_min) and ke_min >= 0.0):
        raise ValueError("ke_min must be finite and not negative")
    if not (np.isfinite(bw_scale) and bw_scale > 0.0 and np.isfinite(h_floor) and h_floor > 0.0):
        raise ValueError("bw_scale and h_floor must be finite and positive")
    levels = [float(v) for v in levels]
    if len(levels) > _abi.CASUALTY_MAX_LEVELS or not all(0.0 < v < 1.0 for v in levels):
        raise ValueError(f"at most {_abi.CASUALTY_MAX_LEVELS} levels, each in (0, 1)")
    lib = _abi.load_library()
    spec = _abi.ErplCasualtySpec()
    _abi.check(lib, lib.erpl_mc_casualty_defaults(C.byref(spec)), "erpl_mc_casualty_defaults")
    spec.n_nodes, spec.n_fragments, spec.bins_x, spec.bins_y = n_nodes, len(frags), bins_x, bins_y
    spec.smooth, spec.n_levels, spec.ke_min = int(bool(smooth)), len(levels), ke_min
    spec.lo_x, spec.hi_x, spec.lo_y, spec.hi_y, spec.bw_scale, spec.h_floor = lo_x, hi_x, lo_y, hi_y, bw_scale, h_floor
    for i in range(_abi.CASUALTY_MAX_LEVELS):
        spec.level[i] = levels[i] if i < len(levels) else 0.0
    for f, (pieces, area, mass) in enumerate(frags):
        spec.pieces[f], spec.area[f], spec.mass[f] = pieces, area, mass
    return spec


def casualty_result_dict(spec, res, p_fail, per_node, per_fragment, groups, hazard, words, risk):
    """What erpl_mc_casualty hands back as a dict: m_c and the job counts, ec / ec_std / ec_se / ec_max / ec_max_col, ec_map,
    ec_smooth, mix_mass, q, w_max, cell_area, levels with level_area / level_area_smooth, 'per_node' and 'per_fragment'
    ({'ec', 'landed', 'lethal', 'off_grid', 'missing'} -> NumPy), 'groups' ([rows, 8], _abi.CASUALTY_G_*), 'hazard',
    'hazard_words', 'risk_count' (hazard / cell_area), 'risk_smooth' (None without smoothing), the edges and centres of the
    raster, 'p_fail' and 'missing_share', the share of the jobs of counted columns that carry no landing."""
    K, F, nl = spec.n_nodes, spec.n_fragments, spec.n_levels
    split = lambda a: dict(zip(("ec",) + CASUALTY_COUNTS, (a[i].copy() for i in range(5))))   # noqa: E731
    ex, ey = np.linspace(spec.lo_x, spec.hi_x, spec.bins_x + 1), np.linspace(spec.lo_y, spec.hi_y, spec.bins_y + 1)
    jobs = int(res.m_c) * K * F
    out = {k: int(getattr(res, k)) for k in ("m_c", "landed", "lethal", "off_grid", "missing", "ec_max_col", "q")}
    out.update({k: float(getattr(res, k)) for k in ("ec", "ec_std", "ec_se", "ec_max", "ec_map", "w_max", "cell_area", "ec_smooth",
                                                    "mix_mass")})
    out.update({"n_nodes": K, "n_fragments": F, "levels": list(spec.level[:nl]), "level_area": list(res.level_area[:nl]),
                "level_area_smooth": list(res.level_area_smooth[:nl]), "per_node": split(per_node),
                "per_fragment": split(per_fragment), "groups": groups, "hazard": hazard, "hazard_words": words,
                "risk_count": hazard / float(res.cell_area), "risk_smooth": risk, "edges_x": ex, "edges_y": ey,
                "centres_x": 0.5 * (ex[:-1] + ex[1:]), "centres_y": 0.5 * (ey[:-1] + ey[1:]),
                "ranges": ((spec.lo_x, spec.hi_x), (spec.lo_y, spec.hi_y)), "p_fail": np.asarray(p_fail, dtype=np.float64).copy(),
                "ke_min": float(spec.ke_min), "missing_share": int(res.missing) / jobs if jobs else float("nan")})
    return out


def casualty_expectation(values, fragments, p_fail, population, ranges, mask=None, engine=None, times=None, **kw):
    """The casualty expectation of a debris footprint, assembled on the host around TrajectoryEngine.casualty (its arguments;
    `population` may be a NumPy array, it is uploaded).  On top of that call's dict: 'time' (the node times, if given),
    'population' (the device tensor), 'ec_contribution' [nodes] = p_fail * per_node['ec'] - what every break-up time adds to
    ec - and 'fragment_share' [fragments] = per_fragment['ec'] / ec."""
    import torch
    engine = _engine_of(values, engine)
    if not torch.is_tensor(population):
        population = torch.as_tensor(np.ascontiguousarray(population, dtype=np.float64), device=engine.device)
    out = engine.casualty(values, fragments, p_fail, population.contiguous(), ranges, mask=mask, **kw)
    out["time"] = None if times is None else np.asarray(times, dtype=np.float64).copy()
    out["population"] = population
    out["fragments"] = [tuple(float(v) for v in f) for f in fragments]
    out["ec_contribution"] = out["p_fail"] * out["per_node"]["ec"]
    with np.errstate(invalid="ignore", divide="ignore"):
        out["fragment_share"] = out["per_fragment"]["ec"] / out["ec"]
    return out
