"""The plain NumPy restatement of erpl_mc_casualty (include/erpl_mc.h): every rule of the header once more, as slowly and as
plainly as it reads there.  The serial loop over (k, f) for the trajectory's expectation, np.add.at on int64 for the hazard map,
two-pass moments per group, the mixture of Gaussian kernels evaluated directly.  No device, no library."""
import math

import numpy as np

CH_X, CH_Y, CH_V = 0, 1, 4
Q_MOST, Q_LEAST = 40, 16
TILE, TARGET_BLOCKS = 1024, 1024


def edges(lo, hi, bins):
    return np.linspace(lo, hi, bins + 1)


def centres(lo, hi, bins):
    e = edges(lo, hi, bins)
    return 0.5 * (e[:-1] + e[1:])


def bin_of(x, lo, hi, bins):
    """np.histogram's bin of x in [lo, hi] (f_indices, one step down, one step up against the edges)."""
    x = np.asarray(x, dtype=np.float64)
    e = edges(lo, hi, bins)
    with np.errstate(invalid="ignore", over="ignore"):
        f = ((x - lo) / (hi - lo)) * float(bins)
        k = np.where(f >= float(bins), bins - 1, np.where(f > 0.0, np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0), 0.0)).astype(np.int64)
    k = np.clip(k, 0, bins - 1)
    k = np.where((x < e[k]) & (k > 0), k - 1, k)
    k = np.where((k < bins - 1) & (x >= e[np.minimum(k + 1, bins)]), k + 1, k)
    return k


def q_of(m, n_nodes, n_fragments):
    return min(Q_MOST, 62 - int(m * n_nodes * n_fragments).bit_length())


def weights(p_fail, c, m):
    """w [K, F], w_max, Q and the integer weights W [K, F] of the hazard map."""
    w = np.asarray(p_fail, dtype=np.float64)[:, None] * np.asarray(c, dtype=np.float64)[None, :]
    w_max = float(w.max())
    Q = q_of(m, w.shape[0], w.shape[1])
    W = np.floor((w / w_max) * 2.0 ** Q).astype(np.int64) if w_max > 0.0 else np.zeros(w.shape, dtype=np.int64)
    return w, w_max, Q, W


def slices(rows, cells):
    blocks = (cells + TILE - 1) // TILE
    want = (TARGET_BLOCKS + blocks - 1) // blocks
    most = min(rows, want)
    per = (rows + most - 1) // most
    return (rows + per - 1) // per, per


def casualty(values, m, mask, fragments, p_fail, population, ranges, ke_min=15.0, smooth=True, bw_scale=1.0, h_floor=1.0,
             levels=(1e-6, 1e-5), want_risk=True):
    """values float64 [5, K * F, ld]; mask uint8 [m] or None; fragments [(pieces, area, mass)] * F; p_fail [K]; population
    [bins_x, bins_y]; ranges ((lo_x, hi_x), (lo_y, hi_y)).  Returns the dict TrajectoryEngine.casualty returns."""
    values = np.asarray(values, dtype=np.float64)
    p_fail = np.asarray(p_fail, dtype=np.float64)
    population = np.asarray(population, dtype=np.float64)
    K, F = len(p_fail), len(fragments)
    R = K * F
    assert values.shape[:2] == (5, R)
    bins_x, bins_y = population.shape
    (lo_x, hi_x), (lo_y, hi_y) = ranges
    pieces, area, mass = (np.array([f[i] for f in fragments], dtype=np.float64) for i in range(3))
    c = pieces * area
    counted = np.ones(m, dtype=bool) if mask is None else (np.asarray(mask)[:m] == 0)
    m_c = int(counted.sum())
    X, Y, V = values[CH_X, :, :m].reshape(K, F, m), values[CH_Y, :, :m].reshape(K, F, m), values[CH_V, :, :m].reshape(K, F, m)
    landed = np.isfinite(X) & np.isfinite(Y) & np.isfinite(V)
    with np.errstate(invalid="ignore", over="ignore"):
        lethal = landed & ((0.5 * mass)[None, :, None] * (V * V) >= ke_min)
        inside = lethal & (X >= lo_x) & (X <= hi_x) & (Y >= lo_y) & (Y <= hi_y)
    cell = np.where(inside, bin_of(np.where(inside, X, lo_x), lo_x, hi_x, bins_x) * bins_y
                    + bin_of(np.where(inside, Y, lo_y), lo_y, hi_y, bins_y), 0)
    h = np.where(inside, c[None, :, None] * population.reshape(-1)[cell], 0.0)
    # the trajectory's expectation: the serial loop of the header
    e = np.zeros(m)
    for k in range(K):
        s = np.zeros(m)
        for f in range(F):
            s = s + h[k, f]
        e = e + p_fail[k] * s
    ec_traj = np.where(counted, e, np.nan)
    ej = e[counted]
    out = {"m_c": m_c, "ec_traj": ec_traj}
    nan = float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        out["ec"] = float(ej.sum() / m_c) if m_c else nan
        out["ec_std"] = float(np.sqrt(((ej - out["ec"]) ** 2).sum() / (m_c - 1))) if m_c else nan
        out["ec_se"] = out["ec_std"] / math.sqrt(m_c) if m_c else nan
    out["ec_max"] = float(ej.max()) if m_c else nan
    out["ec_max_col"] = int(np.flatnonzero(counted & (e == out["ec_max"]))[0]) if m_c else -1
    cm = counted[None, None, :]
    cnt = {"landed": landed & cm, "lethal": lethal & cm, "off_grid": lethal & ~inside & cm, "missing": ~landed & cm}
    for name, sel in cnt.items():
        out[name] = int(sel.sum())
    S = np.where(cm, h, 0.0).sum(axis=2)   # [K, F]
    with np.errstate(invalid="ignore", divide="ignore"):
        node = {"ec": np.array([sum(S[k, f] for f in range(F)) for k in range(K)]) / float(m_c)}
        frag = {"ec": np.array([sum(p_fail[k] * S[k, f] for k in range(K)) for f in range(F)]) / float(m_c)}
    for name, sel in cnt.items():
        node[name] = sel.sum(axis=(1, 2)).astype(np.float64)
        frag[name] = sel.sum(axis=(0, 2)).astype(np.float64)
    out["per_node"], out["per_fragment"] = node, frag
    # the hazard map in exact integers
    w, w_max, Q, W = weights(p_fail, c, m)
    M = np.zeros(bins_x * bins_y, dtype=np.int64)
    hit = inside & cm
    np.add.at(M, cell[hit], np.broadcast_to(W[:, :, None], hit.shape)[hit])
    scale = (w_max * 2.0 ** -Q) / float(m_c) if m_c else 0.0
    hazard = M.astype(np.float64) * scale
    cell_area = ((hi_x - lo_x) / float(bins_x)) * ((hi_y - lo_y) / float(bins_y))
    out.update({"q": Q, "w_max": w_max, "hazard_words": M.reshape(bins_x, bins_y), "hazard": hazard.reshape(bins_x, bins_y),
                "cell_area": cell_area, "ec_map": float((hazard * population.reshape(-1)).sum()),
                "level_area": [float(((hazard / cell_area) >= lv).sum()) * cell_area for lv in levels], "levels": list(levels)})
    # the groups
    member = lethal & cm
    groups = np.full((R, 8), np.nan)
    groups[:, 0], groups[:, 1], groups[:, 7] = member.sum(axis=2).reshape(-1), S.reshape(-1), w.reshape(-1)
    out["groups"] = groups
    out["ec_smooth"], out["mix_mass"], out["risk_smooth"], out["level_area_smooth"] = nan, nan, None, [nan] * len(levels)
    if not smooth:
        return out
    gx, gy = centres(lo_x, hi_x, bins_x), centres(lo_y, hi_y, bins_y)
    GX, GY = np.repeat(gx, bins_y), np.tile(gy, bins_x)
    risk = np.zeros(bins_x * bins_y)
    denom = 0.0
    for r in range(R):
        k, f = divmod(r, F)
        px, py = X[k, f][member[k, f]], Y[k, f][member[k, f]]
        n = len(px)
        denom += (w[k, f] * n) / m_c if m_c else 0.0
        if n == 0:
            continue
        mx, my = px.sum() / n, py.sum() / n
        dx, dy = px - mx, py - my
        cov = np.array([(dx * dx).sum(), (dx * dy).sum(), (dy * dy).sum()]) / (n - 1) if n >= 2 else np.zeros(3)
        f2 = (bw_scale * float(n) ** (-1.0 / 6.0)) ** 2
        hxx, hxy, hyy = f2 * cov[0] + h_floor * h_floor, f2 * cov[1], f2 * cov[2] + h_floor * h_floor
        groups[r, 2:7] = mx, my, hxx, hxy, hyy
        if want_risk:
            risk += mixture_term(GX, GY, px, py, (hxx, hxy, hyy), w[k, f] / m_c)
    out["risk_smooth"] = risk.reshape(bins_x, bins_y) if want_risk else None
    if want_risk:
        out["ec_smooth"] = float(((risk * population.reshape(-1)) * cell_area).sum())
        out["mix_mass"] = float((risk * cell_area).sum() / denom) if denom > 0.0 else nan
        out["level_area_smooth"] = [float((risk >= lv).sum()) * cell_area for lv in levels]
    return out


def mixture_term(qx, qy, px, py, H, weight, dtype=np.float64):
    """weight * sum_j exp(-0.5 (q - x_j)' H^-1 (q - x_j)) / (2 pi sqrt(det H)) at the query points, the direct formulation."""
    T = dtype
    hxx, hxy, hyy = (T(v) for v in H)
    det = hxx * hyy - hxy * hxy
    a, b, c = hyy / det, -hxy / det, hxx / det
    out = np.zeros(len(qx), dtype=T)
    step = max(1, 2_000_000 // max(len(qx), 1))
    qx, qy, px, py = (np.asarray(v).astype(T) for v in (qx, qy, px, py))
    for s in range(0, len(px), step):
        dx, dy = qx[:, None] - px[None, s:s + step], qy[:, None] - py[None, s:s + step]
        out += np.exp(T(-0.5) * (a * dx * dx + T(2) * b * dx * dy + c * dy * dy)).sum(axis=1)
    return out * (T(weight) / (T(2) * T(np.pi) * np.sqrt(det)))


def mixture_term_whitened(qx, qy, px, py, H, weight):
    """The same term through the inverse Cholesky factor of H (scipy.stats.gaussian_kde's evaluation)."""
    L = np.linalg.cholesky(np.array([[H[0], H[1]], [H[1], H[2]]], dtype=np.float64))
    Wm = np.linalg.inv(L)
    P, Qm = Wm @ np.vstack([px, py]), Wm @ np.vstack([qx, qy])
    out = np.zeros(len(qx))
    step = max(1, 2_000_000 // max(len(qx), 1))
    for s in range(0, P.shape[1], step):
        du, dv = Qm[0][:, None] - P[0][None, s:s + step], Qm[1][:, None] - P[1][None, s:s + step]
        out += np.exp(-0.5 * (du * du + dv * dv)).sum(axis=1)
    return out * (weight / (2.0 * np.pi * L[0, 0] * L[1, 1]))
