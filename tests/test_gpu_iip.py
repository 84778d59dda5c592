"""erpl_mc_impact_points on a real MI355X (`pytest -m gpu`): the instantaneous impact points of captured trajectories against
tests/iip_ref.py, the plain Python / NumPy restatement of the definitions in include/erpl_mc.h over the CPU oracle.

Bounds.  The NaN pattern (not evaluated, not of physical size, not landed) must be EQUAL.  Finite values hold
|got - exp| <= 1e-9 * max(|exp|, 1): the bound test_gpu_envelope.py and test_extract_histories_vs_oracle hold the same
device functions to; the fall does not amplify it (drag is dissipative).  LANDED, NODES and the node choices of the summary
must be equal; rows that follow an argmax of COMPUTED values (MAX_RANGE, MAX_RATE) are checked at the node the GPU chose,
found from its time: the restated value there must be within the bound of the restated maximum.  Everything that is a copy
or an IEEE operation on stored doubles in a stated order (a start below the ground, the node times) must be equal to the bit.
dt = 0.25 and max_steps = 4000 unless stated: a fall is at most ~600 steps.  Each distinct (sample, parameters, record) is
restated once for the whole module."""
import math

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import helpers as H
import iip_ref
from test_gpu_corridor import check_bands
from test_gpu_envelope import Flights

pytestmark = pytest.mark.gpu

A = _abi
NAN = float("nan")
TOL = 1e-9
DT, MAX_STEPS, STRIDE, NODES = 0.25, 4000, 64, 32
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
    """The restatement of nodes of the `liquid` samples, each distinct (sample, parameters, record) once."""

    def __init__(self, orc, f):
        self.orc, self.f, self.cache, self.falls = orc, f, {}, {}

    def fall(self, sid, **kw):
        key = (sid,) + tuple(sorted(kw.items()))
        if key not in self.falls:
            par = dict(dt=DT, max_steps=MAX_STEPS)
            par.update(kw)
            self.falls[key] = iip_ref.Fall(self.orc, self.f.cfg, self.f.hb.take([sid]), **par)
        return key, self.falls[key]

    def values(self, sid, rec, nodes, stride=STRIDE, **kw):
        key, fall = self.fall(sid, **kw)
        return iip_ref.values_of(fall, rec, nodes, stride, self.cache, key)

    def summary(self, sid, vals, rec, stride=STRIDE, keep_in=None):
        return iip_ref.summary_of(vals, rec, stride, float(self.f.hb.motor[3, sid]), keep_in)


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


def close(got, exp):
    if np.isnan(exp) or np.isnan(got):
        return bool(np.isnan(exp) and np.isnan(got))
    return abs(got - exp) <= TOL * max(abs(exp), 1.0)


def check_values(got, exp, tag):
    """values [5, nodes] of one column against the restatement."""
    assert got.shape == exp.shape
    with np.errstate(invalid="ignore"):
        err = np.abs(got - exp) / np.maximum(np.abs(exp), 1.0)
    print(tag, "landed", int(np.isfinite(exp[0]).sum()), "of", exp.shape[1], "largest relative error", float(np.nanmax(err)) if np.isfinite(err).any() else 0.0)
    assert np.array_equal(np.isnan(got), np.isnan(exp)), (tag, np.isnan(got).sum(), np.isnan(exp).sum())
    for c in range(5):
        for k in range(exp.shape[1]):
            assert close(got[c, k], exp[c, k]), (tag, analysis.IIP_CHANNELS[c], k, got[c, k], exp[c, k])


def check_summary(got, vals_exp, rec, sid, restated, tag, stride=STRIDE, keep_in=None):
    """One summary column against the restatement of its rows on the restated values."""
    exp, pick = restated.summary(sid, vals_exp, rec, stride, keep_in)
    print(tag, "got", [float(v) for v in got])
    print(tag, "exp", [float(v) for v in exp], pick)
    assert got[A.IIP_LANDED] == exp[A.IIP_LANDED] and got[A.IIP_NODES] == exp[A.IIP_NODES], tag
    n_eval = int(exp[A.IIP_NODES])
    rec = np.asarray(rec).reshape(-1, 15)
    ts = np.array([rec[k * stride, 0] - rec[0, 0] for k in range(n_eval)])
    X, Y, R = vals_exp[A.IIP_CH_X], vals_exp[A.IIP_CH_Y], vals_exp[A.IIP_CH_RANGE]

    def node_of(t):
        hit = np.nonzero(ts == t)[0]
        assert len(hit) == 1, (tag, t)
        return int(hit[0])

    # rows that follow an argmax of computed values: at the node the GPU chose
    if pick["far"] < 0:
        assert np.isnan(got[A.IIP_MAX_RANGE:A.IIP_MAX_RANGE_Y + 1]).all(), tag
    else:
        g = node_of(got[A.IIP_MAX_RANGE_TIME])
        assert close(R[g], exp[A.IIP_MAX_RANGE]) and close(got[A.IIP_MAX_RANGE], exp[A.IIP_MAX_RANGE]), (tag, g, pick)
        assert close(got[A.IIP_MAX_RANGE_X], X[g]) and close(got[A.IIP_MAX_RANGE_Y], Y[g]), (tag, g)
    if pick["rate"] < 0:
        assert np.isnan(got[A.IIP_MAX_RATE]) and np.isnan(got[A.IIP_MAX_RATE_TIME]), tag
    else:
        g = node_of(got[A.IIP_MAX_RATE_TIME])
        assert g + 1 < n_eval and np.isfinite(X[g]) and np.isfinite(X[g + 1])
        dx, dy = X[g + 1] - X[g], Y[g + 1] - Y[g]
        assert close(math.sqrt(dx * dx + dy * dy) / (ts[g + 1] - ts[g]), exp[A.IIP_MAX_RATE]), (tag, g, pick)
        assert close(got[A.IIP_MAX_RATE], exp[A.IIP_MAX_RATE]), (tag, g, got[A.IIP_MAX_RATE], exp[A.IIP_MAX_RATE])
    # rows whose node is a comparison on stored doubles: the node must be the same, its time equal to the bit
    for row in (A.IIP_BURNOUT_TIME, A.IIP_EXIT_TIME):
        assert same_bits(got[row], exp[row]), (tag, analysis.IIP_NAMES[row], got[row], exp[row])
    for row in (A.IIP_BURNOUT_X, A.IIP_BURNOUT_Y, A.IIP_APOGEE_X, A.IIP_APOGEE_Y, A.IIP_EXIT_X, A.IIP_EXIT_Y):
        assert close(got[row], exp[row]), (tag, analysis.IIP_NAMES[row], got[row], exp[row])
    return exp, pick


def capture(engine, ids, records):
    """Hand-made captures on the device, as test_gpu_envelope.envelope_of builds them: (ids, traj, traj_len) tensors."""
    m, cap = len(records), max(1, max(len(r) for r in records))
    traj = np.full((m, cap, 15), NAN)
    for j, r in enumerate(records):
        traj[j, :len(r)] = r
    tlen = np.array([len(r) for r in records], dtype=np.int64)
    dev = engine.device
    return (torch.as_tensor(np.asarray(ids, dtype=np.int64), device=dev), torch.as_tensor(traj, device=dev),
            torch.as_tensor(tlen, device=dev))


def run(engine, db, cap, nodes=NODES, stride=STRIDE, **kw):
    par = dict(dt=DT, max_steps=MAX_STEPS)
    par.update(kw)
    vals, summ = engine.impact_points(db, *cap, nodes=nodes, record_stride=stride, **par)
    torch.cuda.synchronize()
    return vals, summ


# ------------------------------------------------------------------------------------------------ 1. real flights
@pytest.fixture(scope="module")
def real(engine, liquid, picks):
    """impact_points on four of the liquid trajectories: (values [5, 32, 4], summary [16, 4]) as NumPy, and the tensors."""
    f = liquid
    engine.set_config(f.cfg)
    idx = torch.as_tensor(picks, device=engine.device)
    cap = (f.ids[idx].contiguous(), f.traj[idx].contiguous(), f.tlen[idx].contiguous())
    vals, summ = run(engine, f.db, cap)
    return vals.cpu().numpy(), summ.cpu().numpy(), cap, vals, summ


def test_real_flights_against_the_restatement(engine, liquid, picks, real, restated):
    f = liquid
    vals, summ = real[0], real[1]
    assert vals.shape == (5, NODES, 4) and summ.shape == (16, 4)
    blown = 0
    for col, j in enumerate(picks):
        rec = f.records(j)
        exp = restated.values(j, rec, NODES)
        check_values(vals[:, :, col], exp, f"liquid[{j}]")
        row, pick = check_summary(summ[:, col], exp, rec, j, restated, f"liquid[{j}]")
        u = iip_ref.usable_prefix(rec)
        assert row[A.IIP_NODES] == min(NODES, -(-u // STRIDE)) > 10 and 0 < row[A.IIP_LANDED] <= row[A.IIP_NODES]
        assert pick["far"] >= 0 and pick["burnout"] >= 0 and pick["rate"] >= 0 and np.isnan(summ[A.IIP_EXIT_TIME, col])
        with np.errstate(all="ignore"):
            if np.max(np.abs(rec[:u, 4:7])) > 1e30:
                blown += 1
                last = int(row[A.IIP_NODES]) - 1
                big = [k for k in range(last + 1) if np.linalg.norm(rec[k * STRIDE, 4:7]) > 1e6]
                assert np.isnan(vals[:, big, col]).all()          # evaluated, not of physical size (none: the check is vacuous)
        assert np.isnan(vals[:, int(row[A.IIP_NODES]):, col]).all()
    assert blown >= 1


# ------------------------------------------------------------------------------------------------ 2. the job mapping
def test_shapes_columns_are_those_of_the_trajectory_alone(engine, liquid, picks, restated):
    f = liquid
    engine.set_config(f.cfg)
    base = {j: f.records(j).copy() for j in picks}
    j0, j1, j2, j3 = picks
    u1 = iip_ref.usable_prefix(base[j1])
    assert u1 > 7 * STRIDE + 1

    def planted(j, r, c, v):
        rec = base[j].copy()
        rec[r, c] = v
        return rec

    unphysical = planted(j1, 3 * STRIDE, 5, 1e37)     # finite, so usable - but no state to fall from
    unphysical[4 * STRIDE, 3] = -2e5
    pool = [(j1, base[j1], "whole"), (j0, base[j0], "blow-up"), (j3, base[j3][:0], "len 0"), (j2, base[j2][:1], "len 1"),
            (j1, base[j1][:7 * STRIDE + 1], "last node on u - 1"), (j1, base[j1][:7 * STRIDE], "last node on u"),
            (j2, planted(j2, 0, 9, NAN), "NaN in record 0"), (j3, planted(j3, 200, 4, NAN), "NaN in record 200"),
            (j2, base[j2], "whole"), (j3, planted(j3, 5 * STRIDE, 0, np.inf), "inf time on node 5"),
            (j1, unphysical, "nodes 3 and 4 not of physical size")]
    alone = {}
    for n_traj, nodes in ((1, 1), (3, 28), (65, 5), (8, 33), (130, 2)):
        order = [(7 * i + 3 * n_traj) % len(pool) for i in range(n_traj)]      # repeated, unsorted
        ids = [pool[p][0] for p in order]
        assert n_traj < 3 or ids != sorted(ids)
        assert n_traj < 8 or len(set(ids)) < len(ids)
        cap = capture(engine, ids, [pool[p][1] for p in order])
        # col0 > 0 and ld > col0 + n_traj: the columns around the window keep the sentinel
        col0, ld = 3, n_traj + 8
        out = torch.full((5, nodes, ld), SENTINEL, dtype=torch.float64, device=engine.device)
        vals, summ = run(engine, f.db, cap, nodes=nodes, out=out, col0=col0)
        assert vals is out
        v, s = vals.cpu().numpy(), summ.cpu().numpy()
        assert (v[:, :, :col0] == SENTINEL).all() and (v[:, :, col0 + n_traj:] == SENTINEL).all()
        assert not (v[:, :, col0:col0 + n_traj] == SENTINEL).any()
        for col, p in enumerate(order):
            sid, rec, note = pool[p]
            tag = f"({n_traj}, {nodes}) column {col}: {note}"
            if (p, nodes) not in alone:
                a_vals, a_summ = run(engine, f.db, capture(engine, [sid], [rec]), nodes=nodes)
                alone[(p, nodes)] = (a_vals.cpu().numpy()[:, :, 0], a_summ.cpu().numpy()[:, 0])
            assert same_bits(v[:, :, col0 + col], alone[(p, nodes)][0]), tag
            assert same_bits(s[:, col], alone[(p, nodes)][1]), tag
            if col < len(pool):   # (every pool entry is among the first columns of the larger shapes)
                exp = restated.values(sid, rec, nodes)
                check_values(v[:, :, col0 + col], exp, tag)
                check_summary(s[:, col], exp, rec, sid, restated, tag)
        by_note = {pool[p][2]: (v[:, :, col0 + col], s[:, col]) for col, p in enumerate(order)}
        for note, (cv, cs) in by_note.items():
            if note in ("len 0", "NaN in record 0"):
                assert np.isnan(cv).all() and cs[A.IIP_NODES] == 0 == cs[A.IIP_LANDED] and np.isnan(cs[:14]).all(), note
            if note == "len 1":
                assert cs[A.IIP_NODES] == 1 and np.isnan(cv[:, 1:]).all()
            if nodes >= 9:
                want = {"last node on u - 1": 8, "last node on u": 7, "NaN in record 200": 4, "inf time on node 5": 5}
                if note in want:
                    assert cs[A.IIP_NODES] == want[note], (note, cs[A.IIP_NODES])
                if note == "last node on u - 1":
                    assert np.isfinite(cv[:, 7]).all() and np.isnan(cv[:, 8:]).all()
                if note == "last node on u":
                    assert np.isfinite(cv[:, 6]).all() and np.isnan(cv[:, 7:]).all()
                if note == "nodes 3 and 4 not of physical size":
                    assert np.isnan(cv[:, 3:5]).all() and np.isfinite(cv[:, 2]).all() and np.isfinite(cv[:, 5]).all()
                    assert cs[A.IIP_NODES] == min(nodes, -(-u1 // STRIDE)) and cs[A.IIP_LANDED] <= cs[A.IIP_NODES] - 2


# ------------------------------------------------------------------------------------------------ 3. the rules
def test_rules_max_steps_ground_drag_wind_and_precision(engine, liquid, picks, real, restated):
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    f = liquid
    engine.set_config(f.cfg)
    j = picks[1]
    rec = f.records(j)
    cap = tuple(t[1:2].contiguous() for t in real[2])
    few = 12
    # max_steps = 10: 2.5 s of fall.  The last 600 records of the flight, the descent: high nodes do not land, low ones do
    u = iip_ref.usable_prefix(rec)
    tail = rec[u - 600:u]
    vals, summ = run(engine, f.db, capture(engine, [j], [tail]), nodes=25, stride=24, max_steps=10)
    v, s = vals.cpu().numpy()[:, :, 0], summ.cpu().numpy()[:, 0]
    exp = restated.values(j, tail, 25, stride=24, max_steps=10)
    check_values(v, exp, "max_steps 10")
    check_summary(s, exp, tail, j, restated, "max_steps 10", stride=24)
    assert s[A.IIP_NODES] == 25 and 0 < s[A.IIP_LANDED] < s[A.IIP_NODES]
    # drag only slows a descent and g <= g0: a node that stays above the ground for 2.5 s even in vacuum cannot land
    z, vz = tail[::24, 3][:25], tail[::24, 6][:25]
    high = z + np.minimum(vz, 0.0) * 2.5 - 0.5 * 9.81 * 2.5 * 2.5 > 0.0
    assert high.sum() >= 5 and np.isnan(v[0][high]).all() and np.isfinite(v[0, -1])
    # a ground plane above some records: those nodes are their own impact points, to the bit
    ground = 1500.0
    vals, _ = run(engine, f.db, cap, nodes=few, stride=2 * STRIDE, ground=ground)
    v = vals.cpu().numpy()[:, :, 0]
    check_values(v, restated.values(j, rec, few, stride=2 * STRIDE, ground=ground), "ground 1500")
    low = [k for k in range(few) if k * 2 * STRIDE < len(rec) and rec[k * 2 * STRIDE, 3] <= ground]
    high = [k for k in range(few) if k * 2 * STRIDE < len(rec) and rec[k * 2 * STRIDE, 3] > ground]
    assert low and high
    for k in low:
        r = rec[k * 2 * STRIDE]
        assert same_bits(v[[A.IIP_CH_X, A.IIP_CH_Y, A.IIP_CH_TFALL], k], [r[1], r[2], 0.0]), k
        assert close(v[A.IIP_CH_VIMPACT, k], math.sqrt((r[4] * r[4] + r[5] * r[5]) + r[6] * r[6])), k
    assert (v[A.IIP_CH_TFALL, high] > 0.0).all()
    # drag_scale 0 (vacuum: the fall is longer in range) and 2; a batch without a wind table
    ref_vals = real[0][:, ::2, 1][:, :few]
    for tag, kw, db in (("drag_scale 0", dict(drag_scale=0.0), f.db), ("drag_scale 2", dict(drag_scale=2.0), f.db),
                        ("no wind table", dict(wind=False), DeviceBatch(f.db.ic, f.db.rocket, f.db.motor, None, None, _abi.PREC_F64))):
        gpu_kw = {k: val for k, val in kw.items() if k != "wind"}
        vals, _ = run(engine, db, cap, nodes=few, stride=2 * STRIDE, **gpu_kw)
        v = vals.cpu().numpy()[:, :, 0]
        check_values(v, restated.values(j, rec, few, stride=2 * STRIDE, **kw), tag)
        both = np.isfinite(v[0]) & np.isfinite(ref_vals[0])
        assert both.sum() >= 4 and not same_bits(v[:, both], ref_vals[:, both]), tag
    # a PREC_F64_FAST batch is accepted and reads the same fp64 tables: the same bytes
    dbf = DeviceBatch.from_host(f.hb, engine.device, _abi.PREC_F64_FAST)
    vals, summ = run(engine, dbf, real[2])
    assert torch.equal(vals.view(torch.int64), real[3].view(torch.int64))
    assert torch.equal(summ.view(torch.int64), real[4].view(torch.int64))
    with pytest.raises(_abi.ErplError, match=r"rc=-1.*precision"):
        run(engine, DeviceBatch.from_host(f.hb, engine.device, _abi.PREC_F32), real[2])


# ------------------------------------------------------------------------------------------------ 4. the keep-in area
def test_keep_in_area(engine, liquid, picks, real, restated):
    f = liquid
    engine.set_config(f.cfg)
    col = 1
    j = picks[col]
    rec = f.records(j)
    exp = restated.values(j, rec, NODES)
    X, Y = exp[A.IIP_CH_X], exp[A.IIP_CH_Y]
    landed = np.nonzero(np.isfinite(X))[0]
    # the edge x = mid between the restated IIPs of two consecutive landed nodes k, k + 1: every landed node before them is on
    # the side of node k, and NO landed node is within 1 m of the edge - no tested point is near an edge by construction
    box, found = 1e7, None
    for a, b in zip(landed[:-1], landed[1:]):
        mid = 0.5 * (X[a] + X[b])
        side = 1.0 if X[b] > X[a] else -1.0
        before = landed[landed <= a]
        if b == a + 1 and (side * (X[before] - mid) < 0).all() and (np.abs(X[landed] - mid) >= 1.0).all():
            found = (int(a), mid, side)
            break
    assert found is not None
    k, mid, side = found
    keep = [(-box, -box), (mid, -box), (mid, box), (-box, box)] if side > 0 else [(mid, -box), (box, -box), (box, box), (mid, box)]
    for n in landed:
        assert abs(X[n] - mid) >= 1.0 and box - abs(Y[n]) >= 1.0 and box - abs(X[n]) >= 1.0, n
    cap = tuple(t[col:col + 1].contiguous() for t in real[2])
    vals, summ = run(engine, f.db, cap, keep_in=keep)
    s = summ.cpu().numpy()[:, 0]
    assert same_bits(vals.cpu().numpy()[:, :, 0], real[0][:, :, col])             # the polygon changes no value
    row, pick = check_summary(s, exp, rec, j, restated, "keep-in", keep_in=keep)
    assert pick["exit"] == k + 1 and s[A.IIP_EXIT_TIME] == rec[(k + 1) * STRIDE, 0] - rec[0, 0]
    assert same_bits(s[:A.IIP_EXIT_TIME], real[1][:A.IIP_EXIT_TIME, col]) and same_bits(s[A.IIP_LANDED:], real[1][A.IIP_LANDED:, col])
    # a polygon that holds everything, given clockwise and as a triangle: no exit; so does no polygon (test 1)
    for poly in ([(-box, -box), (-box, box), (box, box), (box, -box)], [(-box, -box), (3 * box, -box), (-box, 3 * box)]):
        _, summ = run(engine, f.db, cap, keep_in=poly)
        s = summ.cpu().numpy()[:, 0]
        assert np.isnan(s[A.IIP_EXIT_TIME:A.IIP_EXIT_Y + 1]).all() and same_bits(s, real[1][:, col])
    assert np.isnan(real[1][A.IIP_EXIT_TIME:A.IIP_EXIT_Y + 1]).all()


# ------------------------------------------------------------------------------------------------ 5. repeatability
def test_two_calls_return_the_same_bytes(engine, liquid, real):
    engine.set_config(liquid.cfg)
    vals, summ = run(engine, liquid.db, real[2])
    assert torch.equal(vals.view(torch.int64), real[3].view(torch.int64))
    assert torch.equal(summ.view(torch.int64), real[4].view(torch.int64))
    empty = tuple(t[:0].contiguous() for t in real[2])
    vals, summ = run(engine, liquid.db, empty)
    assert tuple(vals.shape) == (5, NODES, 0) and tuple(summ.shape) == (16, 0)
    vals, summ = engine.impact_points(liquid.db, *real[2], nodes=NODES, record_stride=STRIDE, dt=DT, max_steps=MAX_STEPS, summary=False)
    torch.cuda.synchronize()
    assert summ is None and torch.equal(vals.view(torch.int64), real[3].view(torch.int64))


# ------------------------------------------------------------------------------------------------ 6. the layers
def test_corridor_bands_take_the_matrix_as_it_is(engine, liquid):
    f = liquid
    engine.set_config(f.cfg)
    vals, _ = run(engine, f.db, (f.ids, f.traj, f.tlen), nodes=16, stride=2 * STRIDE)
    host = vals.cpu().numpy()
    qs = (0.05, 0.5, 0.95)
    check_bands(engine.corridor_bands(vals, None, quantiles=qs), host, np.ones(8, dtype=bool), qs, "iip bands")
    mask = np.array([0, 1, 0, 0, 4, 0, 0, 0], dtype=np.uint8)
    b = engine.corridor_bands(vals, torch.as_tensor(mask, device=engine.device), quantiles=qs)
    check_bands(b, host, mask == 0, qs, "iip bands, masked")


def test_python_layer_sub_batches_are_windows_of_one_matrix():
    from erpl_monte_carlo_sim_amd import sampling
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    cap = int(np.ceil(mc.max_time / 0.005 / 25)) + 4
    keep = [(-50.0, -1e6), (400.0, -1e6), (400.0, 1e6), (-50.0, 1e6)]
    kw = dict(stride=25, nodes=16, seed=5, planar=True, dt=DT, max_steps=MAX_STEPS, keep_in=keep, quantiles=(0.05, 0.5, 0.95))
    out = mc.impact_point_trace(dict(H.EXAMPLE_IC), 64, capture_bytes=32 * cap * 120 + 119, **kw)
    rs = out["record_stride"]
    assert out["performance"]["sub_batches"] == 2 and rs == (cap - 4) // 16
    vals, iip = out["values"], out["iip_summary"]
    assert tuple(vals.shape) == (5, 16, 64) and tuple(iip.shape) == (16, 64) and vals.is_cuda and iip.dtype == torch.float64
    assert out["channels"] == list(analysis.IIP_CHANNELS) and out["iip_names"] == list(analysis.IIP_NAMES)
    np.testing.assert_array_equal(out["time"], np.arange(16) * (rs * 25 * 0.005))
    eng = shared_engine(None)
    eng.set_config(mc._config())
    for j, (lo, nb) in enumerate(((0, 32), (32, 32))):
        db = sampling.synthetic_dispersions(nb, mc.rocket, mc.motor, mc.wind_model, dict(H.EXAMPLE_IC), eng.device,
                                            precision=_abi.PREC_F64_FAST, seed=5 + 1000003 * j, uncertainty=mc.uncertainty_params,
                                            base_altitude_profile=None, base_wind_profile=None, planar=True, engine=eng)
        summ, status, traj, tlen = eng.run(db, traj_ids=np.arange(nb), traj_stride=25, traj_cap=cap)
        part, part_summ = eng.impact_points(db, eng._keep, traj, tlen, nodes=16, record_stride=rs, dt=DT, max_steps=MAX_STEPS,
                                            keep_in=keep)
        torch.cuda.synchronize()
        assert torch.equal(part.view(torch.int64), vals[:, :, lo:lo + nb].contiguous().view(torch.int64)), j
        assert torch.equal(part_summ.view(torch.int64), iip[:, lo:lo + nb].contiguous().view(torch.int64)), j
        assert torch.equal(summ.view(torch.int64), out["summary"][:, lo:lo + nb].contiguous().view(torch.int64)), j
    # the bands and the statistics are those of the layers below on the same matrix and mask
    why = out["reasons"]
    b = eng.corridor_bands(vals, why, quantiles=(0.05, 0.5, 0.95))
    for c, name in enumerate(analysis.IIP_CHANNELS):
        for k in ("count", "mean", "std", "min", "max", "quantiles"):
            assert same_bits(out[name][k], b[k][c]) if k != "count" else np.array_equal(out[name][k], b[k][c]), (name, k)
    assert H.same_nested(out["statistics"], analysis.impact_point_statistics(iip, why, engine=eng, quantiles=(0.05, 0.5, 0.95)))
    counted = (why == 0).cpu().numpy()
    n_exit = int((counted & np.isfinite(iip[A.IIP_EXIT_TIME].cpu().numpy())).sum())
    print("exit", n_exit, "of", out["n_samples"])
    assert out["exit_count"] == n_exit and 0 <= n_exit <= out["n_samples"] == int(counted.sum()) > 0
    assert out["exit_probability"] == n_exit / out["n_samples"]
    assert out["exit_interval"] == analysis.wilson_interval(n_exit, out["n_samples"], 0.95)
    free = mc.impact_point_trace(dict(H.EXAMPLE_IC), 64, **{**kw, "keep_in": None})
    assert free["performance"]["sub_batches"] == 1 and math.isnan(free["exit_probability"]) and free["exit_count"] == 0
