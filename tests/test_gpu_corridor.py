"""erpl_mc_corridor_resample / erpl_mc_corridor_bands on a real MI355X (`pytest -m gpu`) against a NumPy restatement of the
definitions in include/erpl_mc.h, written from those definitions.

Bounds.  Resample: the six state channels are IEEE operations on stored doubles in a stated order and must be EQUAL bit
for bit (a NaN equals a NaN).  DOWNRANGE and SPEED go through a square root: equal bytes, or, should the device's square
root differ from NumPy's in the last bit, within one np.spacing of NumPy's value (the rule of check_miss in
test_gpu_distributions.py); the worst figure is printed before it is asserted.  Bands: count, min, max, every order_lo /
order_hi, n_counted and the all-NaN row are exact; mean to 1e-12 * mean(|x|), std to 1e-12 * np.std, a quantile to
1e-12 * max(|order_lo|, |order_hi|) - the bar of test_gpu_analysis.py."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, flatten, models

import helpers as H

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOL = 1e-12
ALL = tuple(range(8))
STATE = (_abi.CH_X, _abi.CH_Y, _abi.CH_Z, _abi.CH_VX, _abi.CH_VY, _abi.CH_VZ)
STATE_AT = tuple(ALL.index(c) for c in STATE)   # their places in a matrix of all eight channels
QS = (0.0, 1.0 / 3.0, 0.5, 1.0)
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------------ the restatement
def channel(rec, ch):
    """The channel value of one record [15] (float64 scalars: one rounding per operation, no FMA)."""
    with np.errstate(all="ignore"):
        if ch == _abi.CH_DOWNRANGE:
            return np.sqrt(rec[1] * rec[1] + rec[2] * rec[2])
        if ch == _abi.CH_SPEED:
            return np.sqrt((rec[4] * rec[4] + rec[5] * rec[5]) + rec[6] * rec[6])
        return rec[{_abi.CH_X: 1, _abi.CH_Y: 2, _abi.CH_Z: 3, _abi.CH_VX: 4, _abi.CH_VY: 5, _abi.CH_VZ: 6}[ch]]


def restate_column(rec, length, channels, nodes, t0, dt, hold):
    """One trajectory: rec [cap, 15], its traj_len -> [C, T]."""
    cap = rec.shape[0]
    n = min(max(int(length), 0), cap)
    out = np.full((len(channels), nodes), NAN)
    fin = np.isfinite(rec[:n]).all(axis=1)
    u = n if fin.all() else int(np.argmin(fin))
    if u == 0:
        return out
    ts = rec[:u, 0] - rec[0, 0]
    for k in range(nodes):
        tk = np.float64(t0) + np.float64(k) * np.float64(dt)
        if tk < 0.0:
            continue
        if tk > ts[u - 1]:
            if hold and u == n:
                out[:, k] = [channel(rec[u - 1], c) for c in channels]
            continue
        lo, hi = 0, u
        while hi - lo > 1:
            mid = lo + (hi - lo) // 2
            if ts[mid] <= tk:
                lo = mid
            else:
                hi = mid
        r = lo
        assert 0 <= r < u and ts[r] <= tk and (r == u - 1 or ts[r + 1] > tk)   # (the stamps of every case increase)
        for j, c in enumerate(channels):
            v0 = channel(rec[r], c)
            if r == u - 1:
                out[j, k] = v0
            else:
                with np.errstate(all="ignore"):
                    w = (tk - ts[r]) / (ts[r + 1] - ts[r])
                    out[j, k] = v0 + (channel(rec[r + 1], c) - v0) * w
    return out


def restate(traj, tlen, channels, nodes, t0, dt, hold):
    """[m, cap, 15], [m] -> [C, T, m]."""
    cols = [restate_column(traj[j], tlen[j], channels, nodes, t0, dt, hold) for j in range(len(tlen))]
    return np.stack(cols, axis=2) if cols else np.zeros((len(channels), nodes, 0))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def check_values(got, exp, channels, tag):
    """A resampled matrix [C, T, m] against its restatement, under the bounds of the module docstring."""
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    for j, c in enumerate(channels):
        if c in STATE:
            assert same_bits(got[j], exp[j]), (tag, analysis.CORRIDOR_CHANNEL_NAMES[c], got[j], exp[j])
            continue
        assert np.array_equal(np.isnan(got[j]), np.isnan(exp[j])), (tag, c)
        if same_bits(got[j], exp[j]):
            continue
        ok = ~np.isnan(exp[j])
        worst = float(np.max(np.abs(got[j][ok] - exp[j][ok]) / np.spacing(np.abs(exp[j][ok]))))
        print(f"{tag} {analysis.CORRIDOR_CHANNEL_NAMES[c]}: the device's square root differs from NumPy's, up to {worst} spacings")
        assert worst <= 1.0, (tag, c, worst)


def resample(engine, traj, tlen, channels, nodes, t0, dt, hold, **kw):
    dev = engine.device
    out = engine.corridor_resample(torch.as_tensor(np.ascontiguousarray(traj), device=dev),
                                   torch.as_tensor(np.asarray(tlen, dtype=np.int64), device=dev), channels, nodes, t0, dt,
                                   hold=hold, **kw)
    torch.cuda.synchronize()
    return out


def sorted_with_zeros(vals):
    """np.sort with -0.0 before +0.0: the order of the selection's keys (it returns a value of the row, sign included).
    The zeros are counted in `vals`: np.sort's min / max networks do not keep the number of negative zeros."""
    rs = np.sort(vals)
    zero = rs == 0.0
    neg = int(np.sum(np.signbit(vals[vals == 0.0])))
    rs[zero] = [-0.0] * neg + [0.0] * (int(zero.sum()) - neg)
    return rs


def check_bands(b, matrix, keep, qs, tag):
    """The dict of engine.corridor_bands against NumPy on the host copy `matrix` [C, T, m] and the counted columns `keep`."""
    n_ch, nodes, _ = matrix.shape
    assert b["n_counted"] == int(keep.sum()) and b["q"] == [float(q) for q in qs]
    assert b["count"].shape == (n_ch, nodes) and b["quantiles"].shape == (n_ch, len(qs), nodes)
    for c in range(n_ch):
        for k in range(nodes):
            row = matrix[c, k]
            vals = row[keep & np.isfinite(row)]
            got = {name: b[name][c, k] for name in ("count", "mean", "std", "min", "max")}
            print(tag, c, k, "count", len(vals), got)
            assert got["count"] == len(vals), (tag, c, k)
            if len(vals) == 0:
                assert all(np.isnan(got[name]) for name in ("mean", "std", "min", "max")), (tag, c, k)
                assert np.isnan(b["quantiles"][c, :, k]).all() and np.isnan(b["order_lo"][c, :, k]).all()
                assert np.isnan(b["order_hi"][c, :, k]).all()
                continue
            rs = sorted_with_zeros(vals)
            assert got["min"] == rs[0] and got["max"] == rs[-1], (tag, c, k)
            assert abs(got["mean"] - vals.mean()) <= TOL * np.mean(np.abs(vals)), (tag, c, k, got["mean"], vals.mean())
            assert abs(got["std"] - vals.std()) <= TOL * vals.std(), (tag, c, k, got["std"], vals.std())
            for i, q in enumerate(qs):
                pos = q * (len(rs) - 1)
                lo = int(np.floor(pos))
                hi = min(lo + 1, len(rs) - 1)
                assert same_bits(b["order_lo"][c, i, k], rs[lo]) and same_bits(b["order_hi"][c, i, k], rs[hi]), (tag, c, k, q)
                exp = rs[lo] + (rs[hi] - rs[lo]) * (pos - lo)
                assert abs(b["quantiles"][c, i, k] - exp) <= TOL * max(abs(rs[lo]), abs(rs[hi])), (tag, c, k, q)


def same_band_bytes(a, b):
    return all(same_bits(a[k], b[k]) for k in ("mean", "std", "min", "max", "quantiles", "order_lo", "order_hi")) and \
        np.array_equal(a["count"], b["count"]) and a["n_counted"] == b["n_counted"]


# ------------------------------------------------------------------------------------------------ resample: hand-made captures
def small_capture():
    """cap = 6: record times 0.5 + {0, 0.25, 0.625, 1, 1.5, 2} (all differences exact), random states."""
    rng = np.random.default_rng(11)
    ts = np.array([0.0, 0.25, 0.625, 1.0, 1.5, 2.0])
    lens = [0, 1, -3, 9, 6, 6, 6, 4]
    traj = rng.normal(size=(len(lens), 6, 15)) * 100.0
    traj[:, :, 0] = 0.5 + ts
    traj[4, 2, 9] = NAN          # u = 2
    traj[5, 2, 0] = np.inf       # u = 2, in the time column
    traj[7, 4:, :] = NAN         # behind len = 4: never read
    return traj, np.array(lens, dtype=np.int64), ts


@pytest.mark.parametrize("hold", (False, True))
def test_resample_small_captures(engine, hold):
    traj, lens, ts = small_capture()
    # nodes at -0.5, -0.25, 0, 0.25, .. 2.25: below 0, on record times (0, 0.25, 1, 1.5), between records, on the last
    # record (2.0) and behind it
    got = resample(engine, traj, lens, ALL, 12, -0.5, 0.25, hold).cpu().numpy()
    exp = restate(traj, lens, ALL, 12, -0.5, 0.25, hold)
    check_values(got, exp, ALL, f"grid hold={hold}")
    assert np.isnan(got[:, :2, :]).all()                       # t_k < 0
    assert np.isnan(got[:, :, [0, 2]]).all()                   # len 0 and len -3
    full = 6                                                   # the full trajectory
    for node, r in ((2, 0), (3, 1), (6, 3), (8, 4), (10, 5)):  # a node on a record time is the record, bit for bit
        for j, c in enumerate(ALL):
            if c in STATE:
                assert same_bits(got[j, node, full], channel(traj[full, r], c)), (node, r, c)
    assert np.isnan(got[:, 11, full]).all() != hold            # behind the end: NaN, or the last value
    assert same_bits(got[:, 10, 3][list(STATE_AT)], [channel(traj[3, 5], c) for c in STATE])   # len 9 is clamped to 6
    for j in (4, 5):                                           # cut off in record 2: u = 2, nothing behind ts(1), never held
        assert not np.isnan(got[:, 2:4, j]).any() and np.isnan(got[:, 4:, j]).all()
    assert not np.isnan(got[:, 2:7, 7]).any() and np.isnan(got[:, 7:, 7]).all() != hold   # len 4: the end is ts = 1.0
    assert not np.isnan(got[:, 2, 1]).any() and np.isnan(got[:, 3:, 1]).all() != hold     # len 1: the end is ts = 0
    # one node, one nextafter past the last record: NaN; with hold the last value iff u == len
    for t_last, cols in ((2.0, (3, full)), (1.0, (7,)), (0.0, (1,))):
        t0 = float(np.nextafter(t_last, np.inf))
        g = resample(engine, traj, lens, ALL, 1, t0, 1.0, hold).cpu().numpy()
        check_values(g, restate(traj, lens, ALL, 1, t0, 1.0, hold), ALL, f"past {t_last} hold={hold}")
        for j in cols:
            assert np.isnan(g[:, 0, j]).all() != hold, (t_last, j)
        assert np.isnan(g[:, 0, [0, 2]]).all() and (t_last == 0.0 or np.isnan(g[:, 0, [4, 5]]).all())
        # and exactly on it: the record itself
        g = resample(engine, traj, lens, STATE, 1, t_last, 1.0, hold).cpu().numpy()
        for j in cols:
            last = min(max(int(lens[j]), 0), 6) - 1
            assert same_bits(g[:, 0, j], [channel(traj[j, last], c) for c in STATE]), (t_last, j)


def long_capture():
    """cap = 300, unevenly spaced stamps, lengths that end inside and behind the grid."""
    rng = np.random.default_rng(12)
    m, cap = 5, 300
    traj = rng.normal(size=(m, cap, 15)) * 1000.0
    traj[:, :, 0] = 3.7 + np.cumsum(rng.uniform(0.01, 0.2, size=(m, cap)), axis=1)
    lens = np.array([300, 257, 100, 300, 2], dtype=np.int64)
    traj[3, 200, 5] = -np.inf    # u = 200
    return traj, lens


@pytest.mark.parametrize("hold", (False, True))
def test_resample_more_nodes_than_threads(engine, hold):
    traj, lens = long_capture()
    t_end = float((traj[:, :, 0] - traj[:, :1, 0]).max())
    t0, dt = 0.013, t_end / 250.0          # 257 nodes: a second node for thread 0, the last ones behind every end
    got = resample(engine, traj, lens, ALL, 257, t0, dt, hold).cpu().numpy()
    check_values(got, restate(traj, lens, ALL, 257, t0, dt, hold), ALL, f"cap 300 hold={hold}")
    assert np.isnan(got[:, -1, :]).all() != hold
    if hold:
        assert np.isnan(got[:, -1, 3]).all() and not np.isnan(got[:, -1, [0, 1, 2, 4]]).any()   # the cut-off one never holds


def test_resample_windows_of_one_matrix(engine):
    traj, lens = long_capture()
    m, a, ld = 5, 2, 9
    chans, nodes, t0, dt = (_abi.CH_Z, _abi.CH_SPEED, _abi.CH_VX), 40, 0.0, 0.5
    whole = resample(engine, traj, lens, chans, nodes, t0, dt, True)
    assert tuple(whole.shape) == (3, nodes, m)
    mat = torch.full((3, nodes, ld), SENTINEL, dtype=torch.float64, device=engine.device)
    out = resample(engine, traj[:a], lens[:a], chans, nodes, t0, dt, True, out=mat, col0=0)
    assert out is mat and bool((mat[:, :, a:] == SENTINEL).all())
    resample(engine, traj[a:], lens[a:], chans, nodes, t0, dt, True, out=mat, col0=a)
    assert torch.equal(mat[:, :, :m].contiguous().view(torch.int64), whole.view(torch.int64))
    assert bool((mat[:, :, m:] == SENTINEL).all())             # the padding is never written
    # a window in the middle, nothing else touched; no trajectories: nothing at all
    mat2 = torch.full((3, nodes, ld), SENTINEL, dtype=torch.float64, device=engine.device)
    resample(engine, traj[1:3], lens[1:3], chans, nodes, t0, dt, True, out=mat2, col0=4)
    assert torch.equal(mat2[:, :, 4:6].contiguous().view(torch.int64), whole[:, :, 1:3].contiguous().view(torch.int64))
    assert bool((mat2[:, :, :4] == SENTINEL).all()) and bool((mat2[:, :, 6:] == SENTINEL).all())
    resample(engine, traj[:0], lens[:0], chans, nodes, t0, dt, True, out=mat2, col0=9)
    assert bool((mat2[:, :, :4] == SENTINEL).all()) and bool((mat2[:, :, 6:] == SENTINEL).all())
    with pytest.raises(ValueError, match="fit"):
        resample(engine, traj, lens, chans, nodes, t0, dt, True, out=mat2, col0=5)


# ------------------------------------------------------------------------------------------------ bands: hand-made matrices
def band_matrix(m, seed):
    """[2, 3, m] and a mask: row (0, 0) normal, (0, 1) few distinct values, (0, 2) both zeros among small values, (1, 0) no
    counted finite value, (1, 1) 300 decades of magnitude with both signs, (1, 2) one value; NaN and +-inf sprinkled in."""
    rng = np.random.default_rng(seed)
    x = np.empty((2, 3, m))
    x[0, 0] = rng.normal(size=m) * 1000.0 + 5000.0
    x[0, 1] = rng.integers(0, 4, size=m).astype(np.float64) * 2.5
    x[0, 2] = rng.choice([-0.0, 0.0, -1.5, 1.5, 2.0 ** -1074], size=m)
    x[1, 1] = rng.choice([-1.0, 1.0], size=m) * 10.0 ** rng.uniform(-150, 150, size=m)   # (the squares stay finite)
    x[1, 2] = 42.125
    mask = (rng.uniform(size=m) < 0.3).astype(np.uint8) * rng.integers(1, 64, size=m).astype(np.uint8)
    if m >= 2:
        mask[0], mask[1] = 0, 7                                # a zero and a non-zero byte whatever was drawn
    else:
        mask[0] = 0
    if m >= 8:
        for c, k in ((0, 0), (0, 1), (0, 2), (1, 1)):
            at = rng.choice(np.arange(2, m), size=max(3, m // 16), replace=False)
            x[c, k, at] = rng.choice([NAN, np.inf, -np.inf], size=len(at))
    x[1, 0] = np.where(mask == 0, rng.choice([NAN, np.inf, -np.inf], size=m), rng.normal(size=m))   # finite only where masked
    return x, mask


@pytest.mark.parametrize("m", (1, 2, 255, 256, 257, 1025, 8193))
def test_bands_against_numpy(engine, m):
    x, mask = band_matrix(m, 100 + m)
    dev = engine.device
    xd, md = torch.as_tensor(x, device=dev), torch.as_tensor(mask, device=dev)
    b = engine.corridor_bands(xd, md, quantiles=QS)
    check_bands(b, x, mask == 0, QS, f"m={m}")
    assert b["count"][1, 0] == 0 and b["count"][0, 0] >= 1
    assert same_band_bytes(b, engine.corridor_bands(xd, md, quantiles=QS))          # a second call: the same bytes
    # ld > m: the padding (finite values that would change every number) is not read
    wide = torch.full((2, 3, m + 5), 7.0e9, dtype=torch.float64, device=dev)
    wide[:, :, :m] = xd
    assert same_band_bytes(b, engine.corridor_bands(wide, md, quantiles=QS, m=m))
    # no mask: every column counts
    free = engine.corridor_bands(xd, None, quantiles=QS)
    check_bands(free, x, np.ones(m, dtype=bool), QS, f"m={m} no mask")
    assert free["n_counted"] == m


def test_bands_without_quantiles_and_refusals(engine):
    x, mask = band_matrix(300, 5)
    xd = torch.as_tensor(x, device=engine.device)
    b = engine.corridor_bands(xd, None, quantiles=())
    check_bands(b, x, np.ones(300, dtype=bool), (), "no q")
    assert b["quantiles"].shape == (2, 0, 3)
    with pytest.raises(_abi.ErplError, match=r"rc=-1.*spec->q\[0\]"):
        engine.corridor_bands(xd, None, quantiles=(1.5,))
    with pytest.raises(_abi.ErplError, match=r"rc=-1.*ld = 300 is below m = 301"):
        engine.corridor_bands(xd, None, m=301)
    with pytest.raises(_abi.ErplError, match=r"rc=-1.*spec->channels\[1\]"):
        engine.corridor_resample(torch.zeros((1, 2, 15), dtype=torch.float64, device=engine.device),
                                 torch.ones(1, dtype=torch.int64, device=engine.device), (0, 9))


# ------------------------------------------------------------------------------------------------ one real capture
def mc_batch(kind, n, planar):
    pl = flatten.generate_parameter_samples(H.UNCERTAINTY, n, stream="seed_i")
    return flatten.dispersed_batch(models.Rocket(), H.make_motor(kind), models.WindModel(), H.EXAMPLE_IC, pl, planar=planar,
                                   base_altitude_profile=H.CSV_ALT, base_wind_profile=H.CSV_WIND)


def test_real_capture(engine):
    """Eight planar liquid flights at stride 25 (the set of test_gpu_envelope.py), resampled and banded."""
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    hb = mc_batch("liquid", 8, True)
    engine.set_config(H.make_config("liquid"))
    db = DeviceBatch.from_host(hb, engine.device, _abi.PREC_F64)
    summ, status, traj, tlen = engine.run(db, traj_ids=list(range(8)), traj_stride=25, traj_cap=2000)
    torch.cuda.synchronize()
    rec, lens, summary = traj.cpu().numpy(), tlen.cpu().numpy(), summ.cpu().numpy()
    assert (lens > 256).all() and (lens <= 2000).all()
    ends = np.array([rec[j, lens[j] - 1, 0] - rec[j, 0, 0] for j in range(8)])
    spec = engine.corridor_spec()
    chans, nodes = list(spec.channels[:spec.n_channels]), spec.n_nodes
    assert chans == [_abi.CH_Z, _abi.CH_DOWNRANGE, _abi.CH_SPEED] and nodes == 256
    dt = float(ends.max()) * 1.02 / (nodes - 1)                # the last node lies behind every landing
    for hold in (False, True):
        vals = engine.corridor_resample(traj, tlen, None, None, 0.0, dt, hold=hold)
        torch.cuda.synchronize()
        got = vals.cpu().numpy()
        check_values(got, restate(rec, lens, chans, nodes, 0.0, dt, hold), chans, f"real hold={hold}")
        b = engine.corridor_bands(vals, None, quantiles=QS)
        check_bands(b, got, np.ones(8, dtype=bool), QS, f"real hold={hold}")
        assert b["count"][0, 0] == 8 and b["count"][0, -1] == (8 if hold else 0)
        if hold:   # the vehicle lies where it landed
            assert same_bits(got[0, -1, :], summary[_abi.SUM_IMPACT_Z])
        assert (np.diff(b["count"][0]) <= 0).all()             # flights only ever leave the population


def test_python_layer(tmp_path):
    from erpl_monte_carlo_sim_amd import plots
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    cap = int(np.ceil(mc.max_time / 0.005 / 25)) + 4
    # three sub-batches (24 + 24 + 16 samples), each resampled into its own window of columns
    out = mc.trajectory_corridor(dict(H.EXAMPLE_IC), 64, stride=25, seed=5, planar=True, capture_bytes=24 * cap * 120 + 119,
                                 nodes=64, quantiles=(0.05, 0.5, 0.95))
    env = mc.flight_envelope(dict(H.EXAMPLE_IC), 64, stride=25, seed=5, planar=True, capture_bytes=24 * cap * 120 + 119)
    assert out["performance"]["sub_batches"] == 3 and out["performance"]["records_per_sample"] == cap
    assert bool(((out["summary"] == env["summary"]) | (out["summary"].isnan() & env["summary"].isnan())).all())
    assert torch.equal(out["status"], env["status"]) and torch.equal(out["reasons"], env["reasons"])
    vals = out["values"]
    assert tuple(vals.shape) == (3, 64, 64) and vals.dtype == torch.float64 and vals.is_cuda
    assert out["channels"] == ["z", "downrange", "speed"] and out["q"] == [0.05, 0.5, 0.95]
    assert out["time"].shape == (64,) and out["time"][0] == 0.0 and out["time"][-1] == pytest.approx(mc.max_time)
    assert out["n_counted"] == out["n_samples"] > 0 and out["n_samples"] + out["n_outliers"] == 64
    eng = shared_engine(None)
    again = analysis.trajectory_corridor(vals, ("z", "downrange", "speed"), 0.0, mc.max_time / 63, quantiles=(0.05, 0.5, 0.95),
                                         mask=out["reasons"], engine=eng)
    for name in out["channels"]:
        assert out[name]["count"].shape == (64,) and out[name]["quantiles"].shape == (3, 64)
        for k in ("count", "mean", "std", "min", "max", "quantiles"):
            assert same_bits(np.asarray(out[name][k], dtype=np.float64), np.asarray(again[name][k], dtype=np.float64)), (name, k)
    # node 0 is the rail exit of every counted sample; with hold every counted sample that ended is still there at the end
    keep = (out["reasons"] == 0).cpu().numpy()
    v = vals.cpu().numpy()
    z0 = v[0, 0, keep]
    assert out["z"]["count"][0] == int(np.isfinite(z0).sum()) and out["z"]["min"][0] == z0[np.isfinite(z0)].min()
    assert out["z"]["count"][-1] == int(np.isfinite(v[0, -1, keep]).sum())
    assert plots.corridor_figure(out) is not None

    class Saver:
        def _create_output_directory(self):
            return str(tmp_path)

    assert plots.plot_trajectory_corridor(Saver(), out) == str(tmp_path)
    assert (tmp_path / "monte_carlo_corridor.png").stat().st_size > 1000
