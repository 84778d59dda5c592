"""Subset simulation as include/erpl_mc.h states it (erpl_mc_subset_*), in NumPy on top of philox_ref and
scipy.special.ndtri: the limit state, the order of the seeds, the proposal, the commit, the chain statistics and the whole
run.  Written from the contract; shares no code with the library.  Normal rows use the exact quantile ndtri(u)."""
import math

import numpy as np
from scipy import special

import philox_ref
from philox_ref import S32

UNIFORM, NORMAL = 0, 1
WHY_NON_FINITE, WHY_APOGEE_HIGH, WHY_APOGEE_LOW, WHY_RANGE, WHY_FLIGHT_TIME, WHY_ENERGY = 1, 2, 4, 8, 16, 32
ST_NAN, ST_INCOMPLETE = 1 << 10, 1 << 11
APOGEE, RANGE, FLIGHT_TIME, IMPACT_X, IMPACT_Y = 0, 4, 5, 8, 9


def limit_state(summary, status, bounds, row=RANGE, sign=1, centre=None):
    """g [n] of summary [16, n]: bounds = (max_apogee, min_apogee, max_range, max_flight_time, energy_apogee)."""
    apo, rng, ft = summary[APOGEE], summary[RANGE], summary[FLIGHT_TIME]
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(apo) & np.isfinite(rng) & np.isfinite(ft))
        bad |= (apo > bounds[0]) | (apo < bounds[1]) | (rng > bounds[2]) | (ft > bounds[3]) | (apo > bounds[4])
        if status is not None:
            bad |= (status & (ST_NAN | ST_INCOMPLETE)) != 0
        if centre is None:
            x = summary[row].copy()
        else:
            dx, dy = summary[IMPACT_X] - centre[0], summary[IMPACT_Y] - centre[1]
            x = np.sqrt(dx * dx + dy * dy)
        bad |= ~np.isfinite(x)
    return np.where(bad, -np.inf, sign * x)


def order_key(g):
    """Ascending in this uint64 key = descending in g; -0.0 below +0.0; NaN as -inf."""
    g = np.where(np.isnan(g), -np.inf, np.asarray(g, dtype=np.float64))
    b = g.view(np.uint64)
    neg = (b >> np.uint64(63)) != 0
    asc = np.where(neg, ~b, b | np.uint64(1 << 63))      # ascending in g
    return ~asc


def seeds(g, n_seeds):
    """(idx ascending, selected uint8, threshold, n_alive)."""
    g = np.asarray(g, dtype=np.float64)
    order = np.lexsort((np.arange(g.size), order_key(g)))
    first = order[:n_seeds]
    sel = np.zeros(g.size, dtype=np.uint8)
    sel[first] = 1
    thr = g[first[-1]]
    return np.sort(first).astype(np.int32), sel, (-np.inf if np.isnan(thr) else thr), int(np.count_nonzero(g > -np.inf))


def uniforms(seed, level, step, rows, first_chain, count):
    """u [rows, count] of the chains first_chain ..: counter (j >> 1, r | t << 16, l, 3)."""
    seed = int(seed)
    j = np.arange(first_chain, first_chain + count, dtype=np.uint64)
    out = np.empty((rows, count))
    for r in range(rows):
        o = philox_ref.philox4x32_10((j >> np.uint64(1), r | (int(step) << 16), int(level), 3), (seed & 0xFFFFFFFF, seed >> 32))
        draw = np.where((j & np.uint64(1)) == 0, o[0] | (o[1] << S32), o[2] | (o[3] << S32))
        u = ((draw >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
        out[r] = np.where(u >= 1.0, np.nextafter(1.0, 0.0), u)
    return out


def propose(cur, kinds, rho, s, w, seed, level, step, first_chain=0):
    """(candidates [R, count], xi [R, count]: ndtri(u) on normal rows, NaN elsewhere)."""
    R, count = cur.shape
    u = uniforms(seed, level, step, R, first_chain, count)
    out, xi = np.empty_like(cur), np.full(cur.shape, np.nan)
    for r in range(R):
        if kinds[r] == NORMAL:
            xi[r] = special.ndtri(u[r])
            out[r] = rho[r] * cur[r] + s[r] * xi[r]
        else:
            v = cur[r] + w[r] * (u[r] - 0.5)
            v = np.where(v < 0.0, v + 1.0, v)
            v = np.where(v >= 1.0, v - 1.0, v)
            v = np.where(v <= 0.0, np.nextafter(0.0, 1.0), v)
            out[r] = np.where(v >= 1.0, np.nextafter(1.0, 0.0), v)
    return out, xi


def normal_bar(cur_row, xi_row, rho, s):
    """The header's bound of a normal row against rho x + s ndtri(u)."""
    return s * 8e-15 * np.maximum(1.0, np.abs(xi_row)) + 2.0 ** -50 * (np.abs(rho * cur_row) + np.abs(s * xi_row))


def chain_stats(sel, chains, steps):
    """(n1, pair [steps - 1]) by the double loop over chains and steps."""
    I = (np.asarray(sel).reshape(steps, chains) != 0).astype(np.int64)
    pair = np.zeros(max(steps - 1, 0), dtype=np.int64)
    for k in range(1, steps):
        for j in range(chains):
            for t in range(steps - k):
                pair[k - 1] += I[t, j] * I[t + k, j]
    return int(I.sum()), pair


def delta(n1, pair, chains, steps, chained):
    N = chains * steps
    p = n1 / N
    gamma = 0.0
    if chained and 0 < n1 < N:
        for k in range(1, steps):
            gamma += (1.0 - k / steps) * (pair[k - 1] / (N - k * chains) - p * p)
        gamma *= 2.0 / (p * (1.0 - p))
    return p, math.sqrt((1.0 - p) / (p * N) * (1.0 + gamma)), gamma


def run(g_of, draws0, kinds, chains, steps, target, rho=0.8, seed=0, max_levels=12):
    """The whole run on NumPy arrays; returns probability, cov, per-level counts n1 and thresholds, evaluations."""
    R, N = draws0.shape
    rho_r = np.full(R, rho)
    s_r = np.sqrt(1.0 - rho_r * rho_r)
    pop, g = draws0, g_of(draws0)
    P, d2, n1s, thresholds, evaluations = 1.0, 0.0, [], [], N
    for level in range(max_levels):
        idx, sel, thr, alive = seeds(g, chains)
        assert alive >= chains
        if thr >= target:
            sel = (g >= target).astype(np.uint8)
        n1, pair = chain_stats_fast(sel, chains, steps)
        p, dl, _ = delta(n1, pair, chains, steps, level > 0)
        P, d2 = P * p, d2 + dl * dl
        n1s.append(n1)
        thresholds.append(float(min(thr, target)) if thr >= target else float(thr))
        if thr >= target:
            return {"probability": P, "cov": math.sqrt(d2), "n1": n1s, "thresholds": thresholds, "evaluations": evaluations}
        nxt, g_nxt = np.empty_like(pop), np.empty_like(g)
        nxt[:, :chains], g_nxt[:chains] = pop[:, idx], g[idx]
        for t in range(1, steps):
            a, b = (t - 1) * chains, t * chains
            cand, _ = propose(nxt[:, a:b], kinds, rho_r, s_r, s_r, seed, level + 1, t)
            gc = g_of(cand)
            evaluations += chains
            take = gc >= thr
            nxt[:, b:b + chains] = np.where(take, cand, nxt[:, a:b])
            g_nxt[b:b + chains] = np.where(take, gc, g_nxt[a:b])
        pop, g = nxt, g_nxt
    raise AssertionError("the target was not reached")


def chain_stats_fast(sel, chains, steps):
    """chain_stats vectorised over the chains (the run above calls it once per level)."""
    I = (np.asarray(sel).reshape(steps, chains) != 0).astype(np.int64)
    return int(I.sum()), np.array([int((I[:steps - k] * I[k:]).sum()) for k in range(1, steps)], dtype=np.int64)
