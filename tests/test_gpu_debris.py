"""erpl_mc_debris on a real MI355X (`pytest -m gpu`): the debris footprint of captured trajectories against
tests/debris_ref.py, the plain Python / NumPy restatement of the definitions in include/erpl_mc.h over the CPU oracle.

Bounds.  The NaN pattern (not evaluated, not of physical size, not landed) must be EQUAL.  Finite values hold
|got - exp| <= 1e-9 * max(|exp|, 1), the bound of test_gpu_iip.py for the same reason: the same device functions, and a fall
under drag is dissipative.  Counts and index choices must be equal; rows that follow an argmax of COMPUTED values are checked
at the job the GPU chose.  dt = 0.25 and max_steps = 20000 unless stated.

The step rule is a discrete decision: the device's pow / exp may differ from the host's in the last bit of the density, and
that can flip m only where k0 * h lies within ~1e-15 of stiff_limit.  Over the ~1e5 steps this module restates that has a
probability of order 1e-10; the first test prints the smallest |k0 * h / stiff_limit - 1| the restatement met.

Nodes.  At stride 64 every node of every flight lies below its usable prefix (the shortest is 1093 records), which would leave
the equality of the NaN patterns without an unevaluated job.  The 6 nodes are therefore 230 records apart: the sixth lies
behind the blow-up's usable prefix.  Each distinct job is restated once for the whole module."""
import math

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import helpers as H
import debris_ref
import iip_ref
from test_gpu_corridor import check_bands
from test_gpu_envelope import Flights

pytestmark = pytest.mark.gpu

A = _abi
NAN, INF = float("nan"), float("inf")
TOL = 1e-9
DT, MAX_STEPS, STRIDE, NODES, SEED = 0.25, 20000, 230, 6, 20240229
FRAGS = ((20.0, 0.0), (200.0, 30.0), (5000.0, 100.0), (INF, 0.0))
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def liquid(engine):
    return Flights(engine, "liquid", True, _abi.PREC_F64, 25, 2000)


class Restated:
    """The restatement of jobs of the `liquid` samples, each distinct (sample, parameters, record, fragment) once."""

    def __init__(self, orc, f):
        self.orc, self.f, self.cache, self.falls, self.stats = orc, f, {}, {}, {}

    def fall(self, sid, **kw):
        key = (sid,) + tuple(sorted(kw.items()))
        if key not in self.falls:
            par = dict(dt=DT, max_steps=MAX_STEPS, seed=SEED)
            par.update(kw)
            self.falls[key] = debris_ref.Fall(self.orc, self.f.cfg, self.f.hb.take([sid]), sid=sid, **par)
        return key, self.falls[key]

    def values(self, sid, rec, nodes, frags=FRAGS, stride=STRIDE, **kw):
        key, fall = self.fall(sid, **kw)
        return debris_ref.values_of(fall, rec, nodes, stride, frags, self.cache, key, self.stats)

    def margin(self):
        return min([f.margin for f in self.falls.values()] + [INF])


@pytest.fixture(scope="module")
def restated(oracle, liquid):
    return Restated(oracle, liquid)


@pytest.fixture(scope="module")
def picks(liquid):
    """Four of the eight trajectories, a blow-up first."""
    with np.errstate(all="ignore"):
        blown = [j for j in range(8) if np.nanmax(np.abs(liquid.records(j)[:, 4:7])) > 1e30]
    assert blown
    return [blown[0]] + [j for j in range(8) if j not in blown][:3]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def close(got, exp):
    if np.isnan(exp) or np.isnan(got):
        return bool(np.isnan(exp) and np.isnan(got))
    return abs(got - exp) <= TOL * max(abs(exp), 1.0)


def check_values(got, exp, tag):
    """values [5, rows] of one column against the restatement."""
    assert got.shape == exp.shape
    with np.errstate(invalid="ignore"):
        err = np.abs(got - exp) / np.maximum(np.abs(exp), 1.0)
    print(tag, "landed", int(np.isfinite(exp[0]).sum()), "of", exp.shape[1], "largest relative error",
          float(np.nanmax(err)) if np.isfinite(err).any() else 0.0)
    assert np.array_equal(np.isnan(got), np.isnan(exp)), (tag, np.isnan(got).sum(), np.isnan(exp).sum())
    for c in range(5):
        for i in range(exp.shape[1]):
            assert close(got[c, i], exp[c, i]), (tag, analysis.DEBRIS_CHANNELS[c], i, got[c, i], exp[c, i])


def check_summary(got, vals_exp, rec, F, tag, stride=STRIDE, keep_in=None):
    """One summary column, all 16 rows, against debris_ref.summary_of on the restated values.  A polygon handed in here has
    no restated impact within 1 m of an edge, so the inside test is the same decision on both sides."""
    exp, pick = debris_ref.summary_of(vals_exp, rec, stride, F, keep_in)
    print(tag, "got", [float(v) for v in got])
    print(tag, "exp", [float(v) for v in exp], pick)
    for row in (A.DEBRIS_LANDED, A.DEBRIS_NODES, A.DEBRIS_OUTSIDE, A.DEBRIS_EXIT_TIME, A.DEBRIS_EXIT_FRAGMENT):
        assert same_bits(got[row], exp[row]), (tag, analysis.DEBRIS_NAMES[row], got[row], exp[row])
    for row in (A.DEBRIS_EXIT_X, A.DEBRIS_EXIT_Y):
        assert close(got[row], exp[row]), (tag, analysis.DEBRIS_NAMES[row], got[row], exp[row])
    n_eval = int(exp[A.DEBRIS_NODES])
    rec = np.asarray(rec).reshape(-1, 15)
    ts = np.array([rec[k * stride, 0] - rec[0, 0] for k in range(n_eval)])
    X, Y, R, TF = (vals_exp[c] for c in (A.IIP_CH_X, A.IIP_CH_Y, A.IIP_CH_RANGE, A.IIP_CH_TFALL))

    def node_of(t):
        hit = np.nonzero(ts == t)[0]
        assert len(hit) == 1, (tag, t)
        return int(hit[0])

    # rows that follow an argmax of computed values: at the job (the node) the GPU chose
    if pick["far"] < 0:
        assert np.isnan(got[A.DEBRIS_MAX_RANGE:A.DEBRIS_MAX_RANGE_FRAGMENT + 1]).all() and np.isnan(got[A.DEBRIS_MAX_TFALL]), tag
        assert np.isnan(got[A.DEBRIS_MAX_TFALL_TIME]) and np.isnan(got[A.DEBRIS_MAX_SPREAD]) and np.isnan(got[A.DEBRIS_MAX_SPREAD_TIME]), tag
        return exp, pick
    f = got[A.DEBRIS_MAX_RANGE_FRAGMENT]
    assert f == int(f) and 0 <= f < F, (tag, f)
    g = node_of(got[A.DEBRIS_MAX_RANGE_TIME]) * F + int(f)
    assert close(R[g], exp[A.DEBRIS_MAX_RANGE]) and close(got[A.DEBRIS_MAX_RANGE], exp[A.DEBRIS_MAX_RANGE]), (tag, g, pick)
    assert close(got[A.DEBRIS_MAX_RANGE_X], X[g]) and close(got[A.DEBRIS_MAX_RANGE_Y], Y[g]), (tag, g)
    k = node_of(got[A.DEBRIS_MAX_TFALL_TIME])
    assert close(got[A.DEBRIS_MAX_TFALL], exp[A.DEBRIS_MAX_TFALL]), (tag, got[A.DEBRIS_MAX_TFALL], exp[A.DEBRIS_MAX_TFALL])
    assert any(close(TF[k * F + ff], exp[A.DEBRIS_MAX_TFALL]) for ff in range(F) if np.isfinite(TF[k * F + ff])), (tag, k, pick)
    k = node_of(got[A.DEBRIS_MAX_SPREAD_TIME])
    on = [k * F + ff for ff in range(F) if np.isfinite(X[k * F + ff])]
    dx, dy = max(X[i] for i in on) - min(X[i] for i in on), max(Y[i] for i in on) - min(Y[i] for i in on)
    assert close(math.sqrt(dx * dx + dy * dy), exp[A.DEBRIS_MAX_SPREAD]), (tag, k, pick)
    assert close(got[A.DEBRIS_MAX_SPREAD], exp[A.DEBRIS_MAX_SPREAD]), (tag, got[A.DEBRIS_MAX_SPREAD], exp[A.DEBRIS_MAX_SPREAD])
    return exp, pick


def capture(engine, ids, records):
    """Hand-made captures on the device: (ids, traj, traj_len) tensors."""
    m, cap = len(records), max(1, max(len(r) for r in records))
    traj = np.full((m, cap, 15), NAN)
    for j, r in enumerate(records):
        traj[j, :len(r)] = r
    tlen = np.array([len(r) for r in records], dtype=np.int64)
    dev = engine.device
    return (torch.as_tensor(np.asarray(ids, dtype=np.int64), device=dev), torch.as_tensor(traj, device=dev),
            torch.as_tensor(tlen, device=dev))


def run(engine, db, cap, frags=FRAGS, nodes=NODES, stride=STRIDE, **kw):
    par = dict(dt=DT, max_steps=MAX_STEPS, seed=SEED)
    par.update(kw)
    vals, summ = engine.debris(db, *cap, frags, nodes=nodes, record_stride=stride, **par)
    torch.cuda.synchronize()
    return vals, summ


# ------------------------------------------------------------------------------------------------ 1. real flights
@pytest.fixture(scope="module")
def real(engine, liquid, picks):
    """debris on four of the liquid trajectories: (values [5, 24, 4], summary [16, 4]) as NumPy, the capture, the tensors."""
    f = liquid
    engine.set_config(f.cfg)
    idx = torch.as_tensor(picks, device=engine.device)
    cap = (f.ids[idx].contiguous(), f.traj[idx].contiguous(), f.tlen[idx].contiguous())
    vals, summ = run(engine, f.db, cap)
    return vals.cpu().numpy(), summ.cpu().numpy(), cap, vals, summ


def test_real_flights_against_the_restatement(engine, liquid, picks, real, restated):
    f, F = liquid, len(FRAGS)
    vals, summ = real[0], real[1]
    assert vals.shape == (5, NODES * F, 4) and summ.shape == (16, 4)
    landed = unevaluated = 0
    for col, j in enumerate(picks):
        rec = f.records(j)
        exp = restated.values(j, rec, NODES)
        check_values(vals[:, :, col], exp, f"liquid[{j}]")
        row, pick = check_summary(summ[:, col], exp, rec, F, f"liquid[{j}]")
        u = iip_ref.usable_prefix(rec)
        assert row[A.DEBRIS_NODES] == min(NODES, -(-u // STRIDE)) and np.isnan(summ[A.DEBRIS_OUTSIDE, col])
        assert np.isnan(vals[:, int(row[A.DEBRIS_NODES]) * F:, col]).all()
        landed += int(row[A.DEBRIS_LANDED])
        unevaluated += (NODES - int(row[A.DEBRIS_NODES])) * F
    # the test's own inputs, through the restatement: the equality of the NaN patterns above is not vacuous
    print("landed", landed, "of", 4 * NODES * F, "unevaluated", unevaluated, "largest m", restated.stats["max_m"], "steps", restated.stats["steps"],
          "smallest |k0 h / limit - 1|", restated.margin())
    assert 2 * landed >= 4 * NODES * F and restated.stats["max_m"] >= 1 and unevaluated >= 1
    assert restated.margin() > 1e-12


# ------------------------------------------------------------------------------------------------ 2. vacuum
def test_no_drag_no_impulse_is_the_impact_point_in_vacuum_to_the_bit(engine, liquid):
    f = liquid
    engine.set_config(f.cfg)
    cap = (f.ids, f.traj, f.tlen)
    got, _ = run(engine, f.db, cap, frags=[(INF, 0.0)], nodes=32, stride=64)
    want, _ = engine.impact_points(f.db, *cap, nodes=32, record_stride=64, dt=DT, max_steps=MAX_STEPS, drag_scale=0.0)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (5, 32, 8) and int(torch.isfinite(want[0]).sum()) >= 64
    assert same_bytes(got, want)
    # the same fragment beside others: its rows of the larger matrix are the same bytes, whatever its index
    both, _ = run(engine, f.db, cap, frags=[(20.0, 0.0), (INF, 0.0)], nodes=32, stride=64)
    assert same_bytes(both[:, 1::2], want) and not same_bytes(both[:, 0::2], want)


# ------------------------------------------------------------------------------------------------ 3. the job mapping
def test_shapes_columns_are_those_of_the_trajectory_alone(engine, liquid, picks, restated):
    f = liquid
    engine.set_config(f.cfg)
    j0, j1, j2, j3 = picks
    base = {j: f.records(j).copy() for j in picks}
    nan_200 = base[j3].copy()
    nan_200[200, 4] = NAN
    pool = [(j1, base[j1], "whole"), (j0, base[j0], "blow-up"), (j3, base[j3][:0], "len 0"), (j2, base[j2][:1], "len 1"),
            (j1, base[j1][:STRIDE + 1], "last node on u - 1"), (j1, base[j1][:STRIDE], "last node on u"),
            (j3, nan_200, "NaN in record 200"), (j2, base[j2], "whole"), (j3, base[j3], "whole")]
    shapes = ((1, 1, ((50.0, 10.0),)), (65, 2, FRAGS[:3]), (130, 1, ((200.0, 30.0), (INF, 0.0))))
    alone = {}
    for n_traj, nodes, frags in shapes:
        F = len(frags)
        order = [(7 * i + 3 * n_traj) % len(pool) for i in range(n_traj)]      # repeated, unsorted
        ids = [pool[p][0] for p in order]
        cap = capture(engine, ids, [pool[p][1] for p in order])
        col0, ld = 3, n_traj + 8
        out = torch.full((5, nodes * F, ld), SENTINEL, dtype=torch.float64, device=engine.device)
        vals, summ = run(engine, f.db, cap, frags=frags, nodes=nodes, out=out, col0=col0)
        assert vals is out
        v, s = vals.cpu().numpy(), summ.cpu().numpy()
        assert (v[:, :, :col0] == SENTINEL).all() and (v[:, :, col0 + n_traj:] == SENTINEL).all()
        assert not (v[:, :, col0:col0 + n_traj] == SENTINEL).any()
        for col, p in enumerate(order):
            sid, rec, note = pool[p]
            tag = f"({n_traj}, {nodes}, {F}) column {col}: {note}"
            if (p, nodes, frags) not in alone:
                a_vals, a_summ = run(engine, f.db, capture(engine, [sid], [rec]), frags=frags, nodes=nodes)
                alone[(p, nodes, frags)] = (a_vals.cpu().numpy()[:, :, 0], a_summ.cpu().numpy()[:, 0])
            assert same_bits(v[:, :, col0 + col], alone[(p, nodes, frags)][0]), tag
            assert same_bits(s[:, col], alone[(p, nodes, frags)][1]), tag
            if col < len(pool):   # (every pool entry is among the first columns of the larger shapes)
                exp = restated.values(sid, rec, nodes, frags)
                check_values(v[:, :, col0 + col], exp, tag)
                check_summary(s[:, col], exp, rec, F, tag)
        by_note = {pool[p][2]: (v[:, :, col0 + col], s[:, col]) for col, p in enumerate(order)}
        for note, (cv, cs) in by_note.items():
            if note == "len 0":
                assert np.isnan(cv).all() and cs[A.DEBRIS_NODES] == 0 == cs[A.DEBRIS_LANDED] and np.isnan(cs[:14]).all(), note
            if note in ("len 1", "last node on u", "NaN in record 200"):
                assert cs[A.DEBRIS_NODES] == 1 and np.isnan(cv[:, F:]).all(), note
            if note == "last node on u - 1" and nodes == 2:
                assert cs[A.DEBRIS_NODES] == 2 and np.isfinite(cv[:, F:]).all(), note
        if n_traj == 65:
            # another seed moves the fragments with an impulse and no others; the same seed in another window: the same bytes
            other, _ = run(engine, f.db, cap, frags=frags, nodes=nodes, seed=SEED + 1)
            o = other.cpu().numpy()
            whole = [c for c, p in enumerate(order) if pool[p][2] == "whole"]
            assert same_bits(o[:, 0::F], v[:, 0::F, col0:col0 + n_traj])                      # fragment 0: dv = 0
            assert not same_bits(o[:, 1::F][:, :, whole], v[:, 1::F, col0:col0 + n_traj][:, :, whole])
            again = torch.full((5, nodes * F, n_traj + 1), SENTINEL, dtype=torch.float64, device=engine.device)
            run(engine, f.db, cap, frags=frags, nodes=nodes, out=again, col0=1)
            assert same_bits(again.cpu().numpy()[:, :, 1:], v[:, :, col0:col0 + n_traj])


# ------------------------------------------------------------------------------------------------ 4. the rules
def test_rules_max_steps_ground_stiffness_and_precision(engine, liquid, picks, real, restated):
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    f = liquid
    engine.set_config(f.cfg)
    j = picks[1]
    rec = f.records(j)
    cap = tuple(t[1:2].contiguous() for t in real[2])
    # max_steps = 10 cuts the falls: the last 600 records of the flight, the descent - high nodes do not land, low ones do
    u = iip_ref.usable_prefix(rec)
    tail = rec[u - 600:u]
    two = ((20.0, 0.0), (INF, 5.0))
    vals, summ = run(engine, f.db, capture(engine, [j], [tail]), frags=two, nodes=25, stride=24, max_steps=10)
    v, s = vals.cpu().numpy()[:, :, 0], summ.cpu().numpy()[:, 0]
    exp = restated.values(j, tail, 25, two, stride=24, max_steps=10)
    check_values(v, exp, "max_steps 10")
    check_summary(s, exp, tail, 2, "max_steps 10", stride=24)
    assert s[A.DEBRIS_NODES] == 25 and 0 < s[A.DEBRIS_LANDED] < 50
    # a ground plane above some records: those jobs are their own impact points, to the bit (no impulse: fragment 0)
    ground, few = 1500.0, 4
    vals, _ = run(engine, f.db, cap, nodes=few, ground=ground)
    v = vals.cpu().numpy()[:, :, 0]
    check_values(v, restated.values(j, rec, few, ground=ground), "ground 1500")
    F = len(FRAGS)
    low = [k for k in range(few) if k * STRIDE < len(rec) and rec[k * STRIDE, 3] <= ground]
    high = [k for k in range(few) if k * STRIDE < len(rec) and rec[k * STRIDE, 3] > ground]
    assert low and high
    for k in low:
        r = rec[k * STRIDE]
        assert same_bits(v[[A.IIP_CH_X, A.IIP_CH_Y, A.IIP_CH_TFALL], k * F], [r[1], r[2], 0.0]), k
    assert (v[A.IIP_CH_TFALL, [k * F for k in high]] > 0.0).all()
    # the stiff fall of DESIGN.md 8.18: 500 m, (250, 0, 100) m/s, beta = 2 - m = 7 is reached and the fragment lands ahead of
    # its start where the restatement says, not 1.2 km behind it as a fixed step would have it
    hand = np.zeros((1, 15))
    hand[0, 1:7] = (0.0, 0.0, 500.0, 250.0, 0.0, 100.0)
    hand[0, 7] = 1.0
    light = ((2.0, 0.0),)
    vals, _ = run(engine, f.db, capture(engine, [j], [hand]), frags=light, nodes=1, stride=1)
    v = vals.cpu().numpy()[:, :, 0]
    key, fall = restated.fall(j)
    exp = np.array(fall.job(hand[0], 0, 0, 2.0, 0.0)).reshape(5, 1)
    print("stiff: got", v[:, 0], "exp", exp[:, 0], "steps", fall.steps, "largest m", fall.max_m)
    check_values(v, exp, "beta 2 from 500 m")
    assert fall.max_m == 7 and fall.steps > 100 and v[A.IIP_CH_X, 0] > 0.0 and v[A.IIP_CH_TFALL, 0] > 60.0
    # stiff_limit = 1 takes other steps: other values, those of its own restatement
    vals, _ = run(engine, f.db, cap, stiff_limit=1.0)
    v = vals.cpu().numpy()[:, :, 0]
    check_values(v, restated.values(j, rec, NODES, stiff_limit=1.0), "stiff_limit 1")
    both = np.isfinite(v[0]) & np.isfinite(real[0][0, :, 1])
    assert both.sum() >= 8 and not same_bits(v[:, both], real[0][:, both, 1])
    # the device draws the host export's directions, bit for bit: a fragment without drag that starts at or below the ground
    # does not fall, so VIMPACT is |v + dv d| in the header's operations and nothing else
    below = np.zeros((1, 15))
    below[0, 1:7] = (3.0, -4.0, -1.0, 120.0, -35.0, 60.0)
    below[0, 7] = 1.0
    kicks = ((INF, 25.0), (INF, 0.0), (INF, 300.0))
    vals, _ = run(engine, f.db, capture(engine, [j], [below]), frags=kicks, nodes=1, stride=1)
    v = vals.cpu().numpy()[:, :, 0]
    for fr, (_, dv) in enumerate(kicks):
        d = analysis.debris_directions(SEED, [j], 0, fr)[:, 0] if dv else np.zeros(3)
        w = [below[0, 4 + c] + dv * d[c] if dv else below[0, 4 + c] for c in range(3)]
        speed = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        assert same_bits(v[:, fr], [3.0, -4.0, 5.0, 0.0, speed]), (fr, v[:, fr], speed, d)
    assert v[A.IIP_CH_VIMPACT, 0] != v[A.IIP_CH_VIMPACT, 1] != v[A.IIP_CH_VIMPACT, 2]
    # a PREC_F64_FAST batch is accepted and reads the same fp64 tables: the same bytes
    dbf = DeviceBatch.from_host(f.hb, engine.device, _abi.PREC_F64_FAST)
    vals, summ = run(engine, dbf, real[2])
    assert same_bytes(vals, real[3]) and same_bytes(summ, real[4])
    with pytest.raises(_abi.ErplError, match=r"rc=-1.*precision"):
        run(engine, DeviceBatch.from_host(f.hb, engine.device, _abi.PREC_F32), real[2])


# ------------------------------------------------------------------------------------------------ 5. the keep-in area
def test_keep_in_area_and_all_summary_rows(engine, liquid, picks, real, restated):
    f, F = liquid, len(FRAGS)
    engine.set_config(f.cfg)
    col = 1
    j = picks[col]
    rec = f.records(j)
    exp = restated.values(j, rec, NODES)
    X, Y = exp[A.IIP_CH_X], exp[A.IIP_CH_Y]
    xs = np.sort(X[np.isfinite(X)])
    # the edge x = mid in the widest gap between the restated impacts: NO impact is within 1 m of it
    gaps = np.diff(xs)
    g = int(np.argmax(gaps))
    assert gaps[g] >= 2.0
    mid, box = 0.5 * (xs[g] + xs[g + 1]), 1e7
    keep = [(-box, -box), (mid, -box), (mid, box), (-box, box)]
    assert (np.abs(xs - mid) >= 1.0).all() and (box - np.abs(Y[np.isfinite(Y)]) >= 1.0).all()
    cap = tuple(t[col:col + 1].contiguous() for t in real[2])
    vals, summ = run(engine, f.db, cap, keep_in=keep)
    s = summ.cpu().numpy()[:, 0]
    assert same_bits(vals.cpu().numpy()[:, :, 0], real[0][:, :, col])             # the polygon changes no value
    row, pick = check_summary(s, exp, rec, F, "keep-in", keep_in=keep)
    n_out = int((xs > mid).sum())
    first = int(np.nonzero(np.isfinite(X) & (X > mid))[0][0])
    assert s[A.DEBRIS_OUTSIDE] == n_out > 0 and pick["exit"] == first and s[A.DEBRIS_EXIT_FRAGMENT] == first % F
    assert s[A.DEBRIS_EXIT_TIME] == rec[(first // F) * STRIDE, 0] - rec[0, 0]
    rest = [r for r in range(16) if r not in (A.DEBRIS_EXIT_TIME, A.DEBRIS_EXIT_FRAGMENT, A.DEBRIS_EXIT_X, A.DEBRIS_EXIT_Y, A.DEBRIS_OUTSIDE)]
    assert same_bits(s[rest], real[1][rest, col])
    # a polygon that holds everything, given clockwise and as a triangle: no exit and a count of 0; no polygon: NaN (test 1)
    for poly in ([(-box, -box), (-box, box), (box, box), (box, -box)], [(-box, -box), (3 * box, -box), (-box, 3 * box)]):
        _, summ = run(engine, f.db, cap, keep_in=poly)
        s = summ.cpu().numpy()[:, 0]
        assert np.isnan(s[A.DEBRIS_EXIT_TIME:A.DEBRIS_EXIT_Y + 1]).all() and s[A.DEBRIS_OUTSIDE] == 0 and same_bits(s[rest], real[1][rest, col])
    assert np.isnan(real[1][A.DEBRIS_EXIT_TIME:A.DEBRIS_EXIT_Y + 1]).all() and np.isnan(real[1][A.DEBRIS_OUTSIDE]).all()


# ------------------------------------------------------------------------------------------------ 6. repeatability, the layers
def test_two_calls_return_the_same_bytes_and_the_layers_take_the_matrix(engine, liquid, real):
    f, F = liquid, len(FRAGS)
    engine.set_config(f.cfg)
    vals, summ = run(engine, f.db, real[2])
    assert same_bytes(vals, real[3]) and same_bytes(summ, real[4])
    empty = tuple(t[:0].contiguous() for t in real[2])
    vals, summ = run(engine, f.db, empty)
    assert tuple(vals.shape) == (5, NODES * F, 0) and tuple(summ.shape) == (16, 0)
    vals, summ = engine.debris(f.db, *real[2], FRAGS, nodes=NODES, record_stride=STRIDE, dt=DT, max_steps=MAX_STEPS, seed=SEED, summary=False)
    torch.cuda.synchronize()
    assert summ is None and same_bytes(vals, real[3])
    # erpl_mc_corridor_bands bands the matrix of all eight flights as it is
    vals, _ = run(engine, f.db, (f.ids, f.traj, f.tlen), frags=FRAGS[:2], nodes=4)
    host = vals.cpu().numpy()
    qs = (0.05, 0.5, 0.95)
    check_bands(engine.corridor_bands(vals, None, quantiles=qs), host, np.ones(8, dtype=bool), qs, "debris bands")
    mask = np.array([0, 1, 0, 0, 4, 0, 0, 0], dtype=np.uint8)
    b = engine.corridor_bands(vals, torch.as_tensor(mask, device=engine.device), quantiles=qs)
    check_bands(b, host, mask == 0, qs, "debris bands, masked")
    # the X and Y rows of one (k, f) are a pair of rows for erpl_mc_histogram_xy: the footprint map of np.histogram2d
    k, fr = 2, 1
    pair = torch.zeros((16, 8), dtype=torch.float64, device=engine.device)
    pair[0], pair[1] = vals[A.IIP_CH_X, k * 2 + fr], vals[A.IIP_CH_Y, k * 2 + fr]
    x, y = host[A.IIP_CH_X, k * 2 + fr], host[A.IIP_CH_Y, k * 2 + fr]
    fin = np.isfinite(x) & np.isfinite(y)
    assert fin.sum() >= 6
    rng = ((float(x[fin].min()) - 1.0, float(x[fin].max()) + 1.0), (float(y[fin].min()) - 1.0, float(y[fin].max()) + 1.0))
    counts, ex, ey, info = engine.histogram2d(pair, None, 0, 1, bins=(6, 5), ranges=rng)
    want, wx, wy = np.histogram2d(x[fin], y[fin], bins=(6, 5), range=rng)
    assert np.array_equal(counts, want.astype(np.int64)) and np.array_equal(ex, wx) and np.array_equal(ey, wy)
    assert info["counted"] == int(fin.sum()) and counts.sum() == fin.sum()


# ------------------------------------------------------------------------------------------------ 7. the Python layer
def test_python_layer_sub_batches_are_windows_of_one_matrix():
    from erpl_monte_carlo_sim_amd import sampling
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    cap = int(np.ceil(mc.max_time / 0.005 / 25)) + 4
    keep = [(-50.0, -1e6), (400.0, -1e6), (400.0, 1e6), (-50.0, 1e6)]
    frags = [(20.0, 10.0), (INF, 0.0)]
    qs = (0.05, 0.5, 0.95)
    kw = dict(fragments=frags, stride=25, nodes=4, seed=5, planar=True, dt=DT, max_steps=MAX_STEPS, keep_in=keep, quantiles=qs,
              maps=[(3, 1)], map_bins=8)
    out = mc.debris_footprint(dict(H.EXAMPLE_IC), 16, capture_bytes=8 * cap * 120 + 119, **kw)
    rs = out["record_stride"]
    assert out["performance"]["sub_batches"] == 2 and rs == (cap - 4) // 4
    vals, deb = out["values"], out["debris_summary"]
    assert tuple(vals.shape) == (5, 8, 16) and tuple(deb.shape) == (16, 16) and vals.is_cuda and deb.dtype == torch.float64
    assert out["channels"] == list(analysis.DEBRIS_CHANNELS) and out["debris_names"] == list(analysis.DEBRIS_NAMES)
    np.testing.assert_array_equal(out["time"], np.arange(4) * (rs * 25 * 0.005))
    eng = shared_engine(None)
    eng.set_config(mc._config())
    for j, (lo, nb) in enumerate(((0, 8), (8, 8))):
        db = sampling.synthetic_dispersions(nb, mc.rocket, mc.motor, mc.wind_model, dict(H.EXAMPLE_IC), eng.device,
                                            precision=_abi.PREC_F64_FAST, seed=5 + 1000003 * j, uncertainty=mc.uncertainty_params,
                                            base_altitude_profile=None, base_wind_profile=None, planar=True, engine=eng)
        summ, status, traj, tlen = eng.run(db, traj_ids=np.arange(nb), traj_stride=25, traj_cap=cap)
        part, part_summ = eng.debris(db, eng._keep, traj, tlen, frags, nodes=4, record_stride=rs, dt=DT, max_steps=MAX_STEPS,
                                     seed=5 + 1000003 * j, keep_in=keep)
        torch.cuda.synchronize()
        assert same_bytes(part, vals[:, :, lo:lo + nb]) and same_bytes(part_summ, deb[:, lo:lo + nb]), j
        assert same_bytes(summ, out["summary"][:, lo:lo + nb]), j
    # the bands, the statistics and the map are those of the layers below on the same matrix and mask
    why = out["reasons"]
    b = eng.corridor_bands(vals, why, quantiles=qs)
    for c, name in enumerate(analysis.DEBRIS_CHANNELS):
        for k in ("count", "mean", "std", "min", "max"):
            assert same_bits(out[name][k], b[k][c].reshape(4, 2)), (name, k)
        assert same_bits(out[name]["quantiles"], b["quantiles"][c].reshape(3, 4, 2)), name
    assert H.same_nested(out["statistics"], analysis.debris_statistics(deb, why, engine=eng, quantiles=qs))
    # ... and every row of the statistics carries its own name: count, mean, min and max against NumPy on the same matrix and
    # mask (a column counts iff a job of it landed; beyond that a row counts its finite values - exit_time only where a
    # fragment left the area)
    dh, counted_cols = deb.cpu().numpy(), (why == 0).cpu().numpy()
    cols = counted_cols & np.isfinite(dh[A.DEBRIS_MAX_RANGE]) & np.isfinite(dh[A.DEBRIS_MAX_RANGE_FRAGMENT]) & np.isfinite(dh[A.DEBRIS_MAX_TFALL])
    assert cols.sum() >= 8
    for r, name in enumerate(analysis.DEBRIS_NAMES):
        st, fin = out["statistics"][name], dh[r, cols][np.isfinite(dh[r, cols])]
        print("statistics", name, st["count"], st["mean"], len(fin), fin.mean() if len(fin) else NAN)
        assert st["count"] == len(fin), (name, st["count"], len(fin))
        if len(fin):
            assert st["min"] == fin.min() and st["max"] == fin.max(), name
            assert abs(st["mean"] - fin.mean()) <= 1e-12 * max(np.abs(fin).mean(), 1.0), (name, st["mean"], fin.mean())
    assert out["statistics"]["max_fall_time"]["count"] == int(cols.sum()) >= out["statistics"]["exit_time"]["count"]
    pair = torch.zeros((16, 16), dtype=torch.float64, device=eng.device)
    pair[0], pair[1] = vals[A.IIP_CH_X, 3 * 2 + 1], vals[A.IIP_CH_Y, 3 * 2 + 1]
    counts, ex, ey, info = eng.histogram2d(pair, why, 0, 1, bins=8)
    m = out["maps"][(3, 1)]
    assert np.array_equal(m["counts"], counts) and np.array_equal(m["edges_x"], ex) and m["info"] == info
    counted = (why == 0).cpu().numpy()
    n_exit = int((counted & np.isfinite(deb[A.DEBRIS_EXIT_TIME].cpu().numpy())).sum())
    print("exit", n_exit, "of", out["n_samples"])
    assert out["exit_count"] == n_exit and 0 <= n_exit <= out["n_samples"] == int(counted.sum()) > 0
    assert out["exit_probability"] == n_exit / out["n_samples"]
    assert out["exit_interval"] == analysis.wilson_interval(n_exit, out["n_samples"], 0.95)
    free = mc.debris_footprint(dict(H.EXAMPLE_IC), 16, **{**kw, "keep_in": None, "maps": ()})
    assert free["performance"]["sub_batches"] == 1 and math.isnan(free["exit_probability"]) and free["exit_count"] == 0
