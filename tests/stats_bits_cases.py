"""The inputs and the calls behind tests/golden/stats_bits.json and stats_host_bits.json: what test_gpu_stats_bits.py
compares and what tools/record_stats_bits.py records.  Only the public TrajectoryEngine calls analyze, histogram,
histogram2d, dispersion and correlation (collect_size) and bootstrap and impact_density (collect_host_size) are used, so
the same code runs on any build of the library.

Every double that a fixed-order reduction produces is kept as the hex pattern of its bits, every integer as it is, bulky
outputs (bin counts, edges, V x V matrices, ranks, the miss distance, the reason bytes) as SHA-256 of their bytes."""
import hashlib
import struct

import numpy as np
import torch

from erpl_monte_carlo_sim_amd import _abi

# n: what it exercises in the reduction
SIZES = (1,             # a single sample
         65,            # a second, ragged wave
         257,           # two workgroups
         1025,          # five partials: thread 0 of the finishing workgroup takes four of them, thread 1 takes one
         262144 + 300)  # the grid saturated at 1 024 partials and a second grid-stride trip for some threads only
# per size, the first seed from 20260 on at which every row used is order_sensitive (below)
SEEDS = {1: 20260, 65: 20264, 257: 20262, 1025: 20260, 262144 + 300: 20260}
ZERO_ROW = _abi.SUM_RAIL_EXIT_SPEED     # non-negative; +0.0 near the front, -0.0 near the end: its minimum is a zero
CORR_ROWS = [ZERO_ROW, _abi.SUM_APOGEE_ALT, _abi.SUM_RANGE]
WIDE_CORR_N, WIDE_CORR_F = 1025, 32     # V = 35 at this one size; V = 5 (two factors) at every size
# the outlier filter of analyze: wide enough to keep most samples, narrow enough that every reason but `energy` counts
BOUNDS = {"max_apogee": 2.0e6, "min_apogee": -2.0e6, "max_range": 1.5e6, "max_flight_time": 1.0e6, "energy_apogee": 1.0e9}


def make_inputs(n):
    """(summary [16, n], factors [32, n], mask uint8 [n], status int32 [n]) of size n, from the legacy generator."""
    rng = np.random.RandomState(SEEDS[n])
    summ = rng.standard_normal((16, n)) * 10.0 ** rng.uniform(-3.0, 6.0, (16, n))
    fac = rng.standard_normal((WIDE_CORR_F, n)) * 10.0 ** rng.uniform(-3.0, 6.0, (WIDE_CORR_F, n))
    mask = ((rng.uniform(size=n) < 0.1) * rng.randint(1, 256, n)).astype(np.uint8)
    status = rng.randint(0, 5, n).astype(np.int32)                  # valid end codes
    status |= ((rng.uniform(size=n) < 0.3) * _abi.ST_APOGEE_LATCHED + (rng.uniform(size=n) < 0.05) * _abi.ST_NAN).astype(np.int32)
    summ[ZERO_ROW] = np.abs(summ[ZERO_ROW])
    if n >= 65:
        summ[ZERO_ROW, 3], summ[ZERO_ROW, n - 2] = 0.0, -0.0
        summ[_abi.SUM_APOGEE_ALT, 10] = np.nan
        summ[_abi.SUM_RANGE, 20] = np.inf
        summ[_abi.SUM_FLIGHT_TIME, 30] = -np.inf
        summ[ZERO_ROW, 40] = np.nan
        summ[_abi.SUM_IMPACT_X, 50] = np.inf
        summ[_abi.SUM_MAX_SPEED, 60] = -np.inf
        fac[0, 61], fac[WIDE_CORR_F - 1, 62] = np.nan, np.inf
        for i in (3, n - 2):                                        # both zeros count in every call
            mask[i] = 0
            status[i] &= ~_abi.ST_NAN
            summ[[_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME], i] = (1.0 + i, 2.0 + i, 3.0 + i)
            summ[[_abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y], i] = (4.0 + i, 5.0 - i)
            fac[:, i] = np.arange(1.0, WIDE_CORR_F + 1.0) * (i + 1.0)
    else:
        mask[:] = 0
    return summ, fac, mask, status


def rows_used(n, summ, fac):
    """The rows some call at size n reduces: the summary and the factors of its correlation calls."""
    return list(summ) + list(fac[:WIDE_CORR_F if n == WIDE_CORR_N else 2])


def order_sensitive(x):
    """Whether three summation orders of the finite values of x disagree: the fixture can tell orders apart."""
    x = x[np.isfinite(x)]
    return not (np.sum(x) == np.cumsum(x)[-1] == np.sum(x[::-1]))


def bits(v):
    """The bit patterns of one double or of a sequence of doubles."""
    if np.ndim(v) == 0:
        return struct.pack(">d", float(v)).hex()
    return [struct.pack(">d", float(x)).hex() for x in np.asarray(v, dtype=np.float64).ravel()]


def digest(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def row_stats(r, nq):
    return {"count": int(r.count), "mean": bits(r.mean), "std": bits(r.std), "min": bits(r.min), "max": bits(r.max),
            "quantile": bits(r.quantile[:nq]), "order_lo": bits(r.order_lo[:nq]), "order_hi": bits(r.order_hi[:nq])}


def correlation_case(engine, fac, summ, mask):
    out = engine.correlation(fac, summ, mask, rows=CORR_ROWS, ranks=True, want_ranks=True)
    rec = {k: int(out[k]) for k in ("count", "n_masked", "n_non_finite")}
    rec.update({k: bits(out[k]) for k in ("mean", "std", "min", "max")})
    rec.update({k: digest(out[k]) for k in ("corr", "rank_corr", "ranks", "pearson", "spearman", "src", "srrc")})
    return rec


def collect_size(engine, n):
    """Every call at size n -> a JSON-ready dict."""
    summ_h, fac_h, mask_h, status_h = make_inputs(n)
    summ, fac, mask, status = (torch.from_numpy(a).to(engine.device) for a in (summ_h, fac_h, mask_h, status_h))
    rec = {}

    res, why = engine.analyze(summ, status, rows=list(range(16)), bounds=BOUNDS, reasons=True)
    nq = engine.analysis_defaults().n_q
    rec["analyze"] = {"n_valid": int(res.n_valid), "n_outliers": int(res.n_outliers),
                      "reason_counts": list(res.reason_counts), "termination_counts": list(res.termination_counts),
                      "n_status_nan": int(res.n_status_nan), "reasons": digest(why),
                      "rows": [row_stats(res.row[r], nq) for r in range(16)]}

    edges, counts, info = engine.histogram(summ, mask, rows=list(range(16)), bins=[17 + 63 * r for r in range(16)])
    rec["histogram"] = {"lo": bits(info["lo"]), "hi": bits(info["hi"]),
                        **{k: [int(c) for c in info[k]] for k in ("counted", "below", "above")},
                        "edges": digest(np.concatenate(edges)), "counts": digest(np.concatenate(counts))}
    rows3 = [_abi.SUM_APOGEE_ALT, ZERO_ROW, _abi.SUM_FLIGHT_TIME]
    edges, counts, info = engine.histogram(summ, mask, rows=rows3, bins=50, ranges=[(-10.0, 10.0), None, (0.0, 1.0e3)])
    rec["histogram_ranges"] = {"lo": bits(info["lo"]), "hi": bits(info["hi"]),
                               **{k: [int(c) for c in info[k]] for k in ("counted", "below", "above")},
                               "counts": digest(np.concatenate(counts))}

    for name, bins, ranges in (("histogram2d_tile", (20, 30), None),                       # cells in LDS
                               ("histogram2d_global", (100, 90), ((-1.0e3, 1.0e3), None))):    # cells in global memory
        counts, ex, ey, info = engine.histogram2d(summ, mask, row_x=_abi.SUM_APOGEE_ALT, row_y=ZERO_ROW, bins=bins,
                                                  ranges=ranges)
        rec[name] = {"counted": int(info["counted"]), "outside": int(info["outside"]),
                     **{k: bits(info[k]) for k in ("lo_x", "hi_x", "lo_y", "hi_y")},
                     "counts": digest(counts), "edges": digest(np.concatenate([ex, ey]))}

    for name, centre in (("dispersion_point", (0.0, 0.0)), ("dispersion_mean", None)):
        d = engine.dispersion(summ, mask, centre=centre, miss=True)
        m = d["miss"]
        rec[name] = {"count": d["count"], "mean": bits(d["mean"]), "covariance": bits(d["covariance"]),
                     "axes": bits([d["var_major"], d["var_minor"], d["angle"]]), "centre": bits(d["centre"]),
                     "inside": [e["inside"] for e in d["ellipses"]],
                     "miss": {"count": m["count"], **{k: bits(m[k]) for k in ("mean", "std", "min", "max", "quantiles",
                                                                                "order_lo", "order_hi")}},
                     "miss_distance": digest(d["miss_distance"])}

    rec["correlation"] = correlation_case(engine, fac[:2].contiguous(), summ, mask)
    if n == WIDE_CORR_N:
        rec["correlation_wide"] = correlation_case(engine, fac, summ, mask)
    return rec


def collect(engine):
    return {str(n): collect_size(engine, n) for n in SIZES}


# ---- stats_host_bits.json: erpl_mc_bootstrap and erpl_mc_impact_density, whose host halves carve one buffer into pieces
HOST_SIZES = (1, 65, 1025, 262144 + 300)    # the last: density alone, several source slices and the largest partial sums
BOOT_SIZES = HOST_SIZES[:3]
BOOT_ROWS = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, _abi.BOOT_ROW_EXTRA]
DENS_NODES = (33, 17)
TRIANGLE = [(-1.0e3, -1.0e3), (2.0e3, 0.0), (0.0, 3.0e3)]
# a 32-gon about (10, -20), vertices rounded to whole metres so that no libm decides a bit of them
GON32 = [(10.0 + float(round(5.0e4 * np.cos(2 * np.pi * k / 32))), -20.0 + float(round(5.0e4 * np.sin(2 * np.pi * k / 32))))
         for k in range(32)]


def bootstrap_case(engine, summ, mask, want_replicates=True, **kw):
    out = engine.bootstrap(summ, mask, replicates=64, seed=7, want_replicates=want_replicates, **kw)
    rec = {k: int(out[k]) for k in ("n", "count", "n_masked", "n_non_finite", "replicates")}

    def stat(s):
        return {"finite": s["finite"], "bits": bits([s[k] for k in ("estimate", "rep_mean", "se", "lo", "hi")])}

    rec["stats"] = [[stat(r["mean"]), stat(r["std"])] + [stat(s) for s in r["quantiles"]] for r in out["stats"]]
    if want_replicates:
        rec["replicate_values"] = digest(out["replicate_values"])
    return rec


def density_case(engine, summ, mask, sample_density=True, **kw):
    d = engine.impact_density(summ, mask, nodes=DENS_NODES, zones=[TRIANGLE, GON32], sample_density=sample_density, **kw)
    sd = d["sample_density_stats"]
    rec = {"count": d["count"], "solid": d["solid"], "peak_node": list(d["peak_node"]),
           "inside": [z["inside"] for z in d["zones"]],
           "moments": bits(d["mean"] + d["covariance"][0] + d["covariance"][1]),
           "bandwidth": bits(d["bandwidth_matrix"][0] + d["bandwidth_matrix"][1] + [d["det"], d["norm"]]),
           "ranges": bits(d["ranges"]), "peak": bits([d["peak"], d["grid_mass"]]), "thresholds": bits(d["thresholds"]),
           "grid": digest(np.concatenate([d["grid_x"], d["grid_y"]])), "density": digest(d["density"]),
           "sample_density_stats": {"count": sd["count"], **{k: bits(sd[k]) for k in ("mean", "std", "min", "max", "quantiles",
                                                                                       "order_lo", "order_hi")}}}
    if sample_density:
        rec["sample_density"] = digest(d["sample_density"])
    return rec


def collect_host_size(engine, n):
    """Every bootstrap and impact_density call at size n -> a JSON-ready dict."""
    summ_h, fac_h, mask_h, _ = make_inputs(n)
    summ, fac, mask = (torch.from_numpy(a).to(engine.device) for a in (summ_h, fac_h, mask_h))
    rec = {}
    if n in BOOT_SIZES:
        extra = fac[0].contiguous()          # holds a NaN from n = 65 on
        rec["bootstrap"] = bootstrap_case(engine, summ, mask, rows=BOOT_ROWS, extra=extra)   # 28 statistics: groups of 16 + 12
        if n == 1025:                        # no summary rows, no quantiles, the replicates in the library's own buffer
            rec["bootstrap_extra_alone"] = bootstrap_case(engine, summ, mask, want_replicates=False, rows=[_abi.BOOT_ROW_EXTRA],
                                                          extra=extra, quantiles=())
        if n == 65:                          # the empty population: every replicate NaN
            rec["bootstrap_empty"] = bootstrap_case(engine, summ, torch.ones_like(mask), rows=BOOT_ROWS, extra=extra)
    rec["density"] = density_case(engine, summ, mask)
    if n == 1025:
        rec["density_no_samples"] = density_case(engine, summ, mask, sample_density=False, levels=())   # no all-pairs pass
        rec["density_explicit"] = density_case(engine, summ, mask, ranges=((-5.0e3, 5.0e3), (-4.0e3, 6.0e3)),
                                               bandwidth=[[4.0e4, 1.0e4], [1.0e4, 9.0e4]])
    if n == 65:                              # row_y constant: not solid, the map is NaN, no error
        flat = summ.clone()
        flat[_abi.SUM_IMPACT_Y] = 3.0
        rec["density_flat"] = density_case(engine, flat, mask)
    return rec


def collect_host(engine):
    return {str(n): collect_host_size(engine, n) for n in HOST_SIZES}
