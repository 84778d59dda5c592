"""NumPy restatement of erpl_mc_corridor_depth, written from the seven sentences of the contract in include/erpl_mc.h (not
from the kernels): np.sort + np.searchsorted per row, a Python loop over the nodes for the sums.  Integer counts are int64,
every floating-point operation is one NumPy operation, so the device has to give the same bits.  `brute_pairs` is the
definition itself - an enumeration of the pairs - for small rows."""
import numpy as np


def c2(n):
    return n * (n - 1) // 2


def populations(values, mask=None, m=None):
    """x [C, T, m] and the membership in_p [C, T, m] of the populations P(c, k) (sentence 1)."""
    values = np.asarray(values, dtype=np.float64)
    m = values.shape[2] if m is None else int(m)
    x = values[:, :, :m]
    counted = np.ones(m, dtype=bool) if mask is None else (np.asarray(mask)[:m] == 0)
    return x, np.isfinite(x) & counted[None, None, :]


def ranks_of_row(xs):
    """a, b (int64) of every member of a population given as its values (sentence 2)."""
    s = np.sort(xs)
    a = np.searchsorted(s, xs, side="left").astype(np.int64)
    b = np.int64(len(xs)) - np.searchsorted(s, xs, side="right").astype(np.int64)
    return a, b


def brute_pairs(xs, j):
    """The pairs {p, q}, p < q, of members (j itself may be one of the two) whose band [min, max] contains xs[j]."""
    cnt = 0
    for p in range(len(xs)):
        for q in range(p + 1, len(xs)):
            cnt += bool(min(xs[p], xs[q]) <= xs[j] <= max(xs[p], xs[q]))
    return cnt


def h_of(central, n_defined):
    if n_defined <= 0:
        return 0
    return int(min(max(np.ceil(np.float64(central) * np.float64(n_defined)), 1.0), float(n_defined)))


def reference(values, mask=None, m=None, central=0.5, factor=1.5):
    x, in_p = populations(values, mask, m)
    C, T, m = x.shape
    factor = np.float64(factor)
    nan = np.float64(np.nan)
    out = {"m": m, "n_masked": 0 if mask is None else int(np.count_nonzero(np.asarray(mask)[:m])),
           "depth": np.full((C, m), nan), "mei": np.full((C, m), nan), "nodes": np.zeros((C, m), np.int32),
           "n_out": np.zeros((C, m), np.int32), "first_out": np.full((C, m), -1, np.int32), "central": np.zeros((C, m), np.uint8),
           "count": in_p.sum(axis=2).astype(np.int64), "n_central_here": np.zeros((C, T), np.int64),
           "n_defined": np.zeros(C, np.int64), "n_central": np.zeros(C, np.int64), "n_outliers": np.zeros(C, np.int64),
           "median": np.full(C, -1, np.int64), "threshold": np.full(C, nan), "depth_max": np.full(C, nan)}
    for name in ("central_lo", "central_hi", "fence_lo", "fence_hi", "whisker_lo", "whisker_hi"):
        out[name] = np.full((C, T), nan)
    with np.errstate(all="ignore"):
        for c in range(C):
            # sentences 2 and 3: one add per counted node, in ascending k
            sd, sm, nodes = np.zeros(m), np.zeros(m), np.zeros(m, np.int32)
            for k in range(T):
                p = in_p[c, k]
                n = np.int64(p.sum())
                if n < 2:
                    continue
                a, b = ranks_of_row(x[c, k, p])
                cov = c2(n) - c2(a) - c2(b)
                sd[p] = sd[p] + cov.astype(np.float64) / np.float64(c2(n))
                sm[p] = sm[p] + (n - a).astype(np.float64) / np.float64(n)
                nodes[p] += 1
            d = nodes > 0
            depth = np.where(d, sd / nodes.astype(np.float64), nan)
            out["depth"][c], out["mei"][c], out["nodes"][c] = depth, np.where(d, sm / nodes.astype(np.float64), nan), nodes
            # sentence 4
            nd = int(d.sum())
            out["n_defined"][c] = nd
            s = np.zeros(m, bool)
            if nd:
                ordered = np.sort(depth[d])
                thr = ordered[nd - h_of(central, nd)]
                s = d & (depth >= thr)
                out["threshold"][c], out["depth_max"][c] = thr, ordered[-1]
                out["median"][c] = np.flatnonzero(d & (depth == ordered[-1]))[0]
            out["central"][c], out["n_central"][c] = s, s.sum()
            # sentence 5
            for k in range(T):
                sel = s & in_p[c, k]
                out["n_central_here"][c, k] = sel.sum()
                if sel.any():
                    lo, hi = x[c, k, sel].min(), x[c, k, sel].max()
                    w = hi - lo
                    reach = factor * w
                    out["central_lo"][c, k], out["central_hi"][c, k] = lo, hi
                    out["fence_lo"][c, k], out["fence_hi"][c, k] = lo - reach, hi + reach
            # sentence 6
            flo, fhi = out["fence_lo"][c][:, None], out["fence_hi"][c][:, None]
            outside = in_p[c] & np.isfinite(flo) & np.isfinite(fhi) & ((x[c] < flo) | (x[c] > fhi))
            n_out = outside.sum(axis=0).astype(np.int32)
            out["n_out"][c] = n_out
            out["first_out"][c] = np.where(n_out > 0, outside.argmax(axis=0), -1)
            out["n_outliers"][c] = (d & (n_out > 0)).sum()
            # sentence 7
            for k in range(T):
                sel = in_p[c, k] & d & (n_out == 0)
                if sel.any():
                    out["whisker_lo"][c, k], out["whisker_hi"][c, k] = x[c, k, sel].min(), x[c, k, sel].max()
    return out


def outliergram_distance(depth, mei, n):
    """d = a0 + a1 mei + a2 n^2 mei^2 - depth (Arribas-Gil & Romo 2014): 0 for a curve that crosses no other."""
    a0 = a2 = -2.0 / (n * (n - 1))
    a1 = 2.0 * (n + 1) / (n - 1)
    return a0 + a1 * mei + a2 * n * n * mei * mei - depth


def demo_curves(n=400, nodes=64, seed=3):
    """The demonstration of the issue: n curves A_i sin(pi t), curve 0 replaced by (1 + 0.12 sin 14 pi t) sin(pi t) (a shape
    outlier inside the pointwise band) and curve 1 by 1.6 sin(pi t) (a magnitude outlier).  Returns values [1, nodes, n]."""
    t = (np.arange(nodes) + 0.5) / nodes
    amp = np.random.default_rng(seed).uniform(0.7, 1.3, n)
    y = amp[None, :] * np.sin(np.pi * t)[:, None]
    y[:, 0] = (1.0 + 0.12 * np.sin(14 * np.pi * t)) * np.sin(np.pi * t)
    y[:, 1] = 1.6 * np.sin(np.pi * t)
    return y[None, :, :].copy()


def make_case(C, T, m, ld, seed=0, integer=False):
    """A test matrix [C, T, ld] with about 2 % NaN, some +-inf, both zeros, 10 % masked columns, a block of columns that ends
    early (ragged populations) and poison behind m; its mask [m]."""
    rng = np.random.default_rng(seed + 1000 * C + 10 * T + m)
    t = np.linspace(0.0, 1.0, T)[None, :, None]
    amp = rng.normal(1.0, 0.2, (C, 1, ld))
    v = amp * np.sin(np.pi * (t + 0.1)) + 0.05 * rng.normal(size=(C, T, ld))
    if integer:
        v = np.round(3.0 * v)
    v[rng.random((C, T, ld)) < 0.02] = np.nan
    v[rng.random((C, T, ld)) < 0.003] = np.inf
    v[rng.random((C, T, ld)) < 0.003] = -np.inf
    z = rng.random((C, T, ld))
    v[z < 0.01] = 0.0
    v[z > 0.99] = -0.0
    first = m // 3
    ends = rng.integers(0, T + 1, size=max(m // 4, 1))
    for i, e in enumerate(ends):   # columns first .. : NaN from node e on
        if first + i < ld:
            v[:, e:, first + i] = np.nan
    v[:, :, m:] = 1e300
    mask = (rng.random(m) < 0.1).astype(np.uint8)
    return v, mask
