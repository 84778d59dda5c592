"""The tests' own restatement of the tally contract (include/erpl_mc.h, erpl_mc_tally_*) in NumPy and plain Python.  It shares
no code with the library: exact sums through math.fsum and fractions.Fraction, bins through np.histogram / np.histogram2d,
quantiles through np.percentile, extremes through a sort by (key, id).

A spec is a plain dict:
  bounds      (max_apogee, min_apogee, max_range, max_flight_time, energy_apogee)
  rows        summary rows; bins, lo, hi, centre: one per row; thresholds: a list per row
  k           extremes held per row and side; percent: the percentiles (the library's q = percent / 100)
  grid        (row_x, row_y, bins_x, bins_y, lo_x, hi_x, lo_y, hi_y); zones: a list of [m, 2] vertex arrays
"""
import math
from fractions import Fraction

import numpy as np

APOGEE_ALT, RANGE, FLIGHT_TIME = 0, 4, 5
ST_NAN, ST_INCOMPLETE = 1 << 10, 1 << 11
BIG, SMALL = 2.0 ** 500, 2.0 ** -485


def reason_bits(bounds, apo, rng, ft):
    """Bit 0 non-finite, 1 apogee high, 2 apogee low (only if not high), 3 range, 4 flight time, 5 energy."""
    max_apogee, min_apogee, max_range, max_ft, energy = bounds
    with np.errstate(invalid="ignore"):
        why = np.zeros(apo.shape, dtype=np.int64)
        why |= (~(np.isfinite(apo) & np.isfinite(rng) & np.isfinite(ft))).astype(np.int64)
        high = apo > max_apogee
        why |= high.astype(np.int64) << 1
        why |= ((~high) & (apo < min_apogee)).astype(np.int64) << 2
        why |= (rng > max_range).astype(np.int64) << 3
        why |= (ft > max_ft).astype(np.int64) << 4
        why |= (apo > energy).astype(np.int64) << 5
    return why


def key_of(values):
    """The order of the extremes: the bit pattern as an unsigned key, -0.0 just below +0.0."""
    b = np.asarray(values, dtype=np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)) != 0
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def inside_polygon(px, py, poly):
    """The even-odd crossing rule, the expression of erpl_mc_impact_density operation by operation."""
    vx, vy = poly[:, 0], poly[:, 1]
    c = np.zeros(px.shape, dtype=bool)
    m = len(poly)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(m):
            j = i - 1 if i > 0 else m - 1
            cond = (vy[i] > py) != (vy[j] > py)
            cross = px < (vx[j] - vx[i]) * (py - vy[i]) / (vy[j] - vy[i]) + vx[i]
            c ^= cond & cross
    return c


def tally(spec, summary, status=None, first_id=0):
    summary = np.asarray(summary, dtype=np.float64)
    n = summary.shape[1]
    ids = first_id + np.arange(n, dtype=np.int64)
    why = reason_bits(spec["bounds"], summary[APOGEE_ALT], summary[RANGE], summary[FLIGHT_TIME])
    valid = why == 0
    out = {"n": n, "n_valid": int(valid.sum()), "reason_counts": [int(((why >> b) & 1).sum()) for b in range(6)],
           "termination_counts": [0] * 5, "n_status_nan": 0, "n_incomplete": 0, "rows": []}
    if status is not None:
        status = np.asarray(status, dtype=np.int64)
        out["termination_counts"] = [int(((status & 0xFF) == c).sum()) for c in range(5)]
        out["n_status_nan"] = int(((status & ST_NAN) != 0).sum())
        out["n_incomplete"] = int(((status & ST_INCOMPLETE) != 0).sum())
    for j, r in enumerate(spec["rows"]):
        x = summary[r]
        use = valid & np.isfinite(x)
        c, cid = x[use], ids[use]
        lo, hi, bins, centre = spec["lo"][j], spec["hi"][j], spec["bins"][j], spec["centre"][j]
        row = {"count": int(c.size), "below": int((c < lo).sum()), "above": int((c > hi).sum()),
               "exceed": [int((c > t).sum()) for t in spec["thresholds"][j]],
               "hist": np.histogram(c[(c >= lo) & (c <= hi)], bins=bins, range=(lo, hi))[0].astype(np.int64)}
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            d = c - np.float64(centre)
            keep = np.abs(d) < BIG      # false for an infinite d too
        row["moment_skipped"] = int((~keep).sum())
        dk = [float(v) for v in d[keep]]
        row["sum_d"] = math.fsum(dk)
        # the exact square, except below 2^-485, where the contract takes the rounded product and nothing else
        exact = sum((Fraction(v) * Fraction(v) if abs(v) >= SMALL else Fraction(v * v) for v in dk), Fraction(0))
        row["sum_d2"] = float(exact)
        if c.size:
            cnt = np.float64(c.size)
            sd, sd2 = np.float64(row["sum_d"]), np.float64(row["sum_d2"])
            with np.errstate(over="ignore", invalid="ignore"):
                md = sd / cnt
                row["mean"] = float(np.float64(centre) + md)
                row["var"] = float((sd2 - sd * md) / cnt)
                row["std"] = float(np.sqrt(np.float64(row["var"])))
        else:
            row["mean"] = row["var"] = row["std"] = math.nan
        keys = key_of(c)
        order = sorted(range(c.size), key=lambda e: (int(keys[e]), int(cid[e])))
        row["sorted"] = c[order]                                  # the counted values in key order
        k = spec["k"]
        row["smallest"] = [(float(c[e]), int(cid[e])) for e in order[:k]]
        back = sorted(range(c.size), key=lambda e: (-int(keys[e]), int(cid[e])))
        row["largest"] = [(float(c[e]), int(cid[e])) for e in back[:k]]
        out["rows"].append(row)
    rx, ry, bx, by, lox, hix, loy, hiy = spec["grid"]
    px, py = summary[rx], summary[ry]
    use = valid & np.isfinite(px) & np.isfinite(py)
    px, py = px[use], py[use]
    inside = (px >= lox) & (px <= hix) & (py >= loy) & (py <= hiy)
    out["grid_counted"], out["grid_outside"] = int(use.sum()), int((~inside).sum())
    out["cells"] = np.histogram2d(px[inside], py[inside], bins=[bx, by], range=[[lox, hix], [loy, hiy]])[0].astype(np.int64)
    out["zone_inside"] = [int(inside_polygon(px, py, np.asarray(z, dtype=np.float64)).sum()) for z in spec["zones"]]
    return out


def virtual_index(count, q):
    """np.percentile's (method='linear') index of the quantile q among `count` sorted values."""
    return np.float64(count - 1) * np.float64(q)


def order_statistics(count, q):
    """The 0-based ranks of the two order statistics behind np.percentile's linear interpolation."""
    v = virtual_index(count, q)
    if v >= count - 1:
        return count - 1, count - 1
    if v < 0:
        return 0, 0
    return int(math.floor(v)), int(math.floor(v)) + 1
