"""erpl_mc_flight_envelope on a real MI355X (`pytest -m gpu`): the envelope of captured trajectories against a NumPy
restatement of the definitions in include/erpl_mc.h.

The restatement takes the per-record quantities from the CPU oracle (oracle.atmosphere, oracle.wind, oracle.extract on the
one-sample batch hb.take([id])) and does windows, argmaxes and the finite-only rule in plain NumPy.

Bounds: USABLE, APOGEE_RECORD and the burnout record are comparisons on the records' own doubles and must be EQUAL, as
must the rows that are IEEE operations on stored doubles in a stated order (BURNOUT_TIME / _ALT / _SPEED, MAX_OMEGA,
MAX_QUAT_DEV).  Rows that go through the atmosphere, the aerodynamic tables and the motor hold
|got - exp| <= 1e-9 * max(|exp|, 1e-300): the bound test_extract_histories_vs_oracle holds the same device functions to.
The rows that follow an argmax of a COMPUTED q are checked at the record the GPU chose (found from MAX_Q_TIME): the oracle's
q there must be within 1e-9 of the oracle's maximum, and MAX_Q_ALT / MAX_Q_MACH are compared with the oracle's values at
that record."""
import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, flatten, models

import helpers as H

pytestmark = pytest.mark.gpu

E = _abi
NAN = float("nan")
EXACT_ROWS = (E.ENV_USABLE, E.ENV_APOGEE_RECORD, E.ENV_BURNOUT_TIME, E.ENV_BURNOUT_ALT, E.ENV_BURNOUT_SPEED, E.ENV_MAX_OMEGA,
              E.ENV_MAX_QUAT_DEV)
VALUE_ROWS = (E.ENV_MAX_Q, E.ENV_MAX_MACH, E.ENV_MAX_Q_ALPHA, E.ENV_MAX_AXIAL_ACCEL, E.ENV_MIN_STABILITY,
              E.ENV_BURNOUT_STABILITY)
TOL = 1e-9


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


def mc_batch(kind, n, planar):
    pl = flatten.generate_parameter_samples(H.UNCERTAINTY, n, stream="seed_i")
    return flatten.dispersed_batch(models.Rocket(), H.make_motor(kind), models.WindModel(), H.EXAMPLE_IC, pl, planar=planar,
                                   base_altitude_profile=H.CSV_ALT, base_wind_profile=H.CSV_WIND)


# ------------------------------------------------------------------------------------------------ the restatement
def first_best(values, window, largest=True):
    """(value, index) of the largest (smallest) FINITE value inside `window`, the lowest index among equals; (NaN, -1)."""
    ok = np.isfinite(values) & window
    if not ok.any():
        return NAN, -1
    keyed = np.where(ok, values if largest else -values, -np.inf)
    i = int(np.argmax(keyed))   # first occurrence
    return float(values[i]), i


def restate(orc, cfg, hb1, rec):
    """The definitions of erpl_mc_flight_envelope for the records rec [len, 15] of the one-sample batch hb1.  Returns
    (envelope [16], per-record dict or None): the dict has ts, z, q, mach, the burnout record b and the max-q record."""
    env = np.full(16, NAN)
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 15)
    fin = np.isfinite(rec).all(axis=1)
    u = len(rec) if fin.all() else int(np.argmin(fin))
    env[E.ENV_USABLE] = u
    if u == 0:
        return env, None
    r = rec[:u]
    ts, z = r[:, 0] - r[0, 0], r[:, 3]
    a = int(np.argmax(z))
    env[E.ENV_APOGEE_RECORD] = a
    late = np.nonzero(ts > hb1.motor[3, 0])[0]
    b = int(late[0]) if len(late) else -1
    ascent, every = np.arange(u) <= a, np.ones(u, dtype=bool)
    with np.errstate(all="ignore"):
        atm = np.array([orc.atmosphere(cfg, float(h)) for h in z])          # T, P, rho, g
        wind = np.array([orc.wind(hb1, float(h)) for h in z])
        diag = orc.extract(cfg, hb1, r, float(r[0, 0]))
        vr = r[:, 4:7] - wind
        vn = np.sqrt((vr[:, 0] * vr[:, 0] + vr[:, 1] * vr[:, 1]) + vr[:, 2] * vr[:, 2])
        mach = vn / np.sqrt((1.4 * 287.053) * atm[:, 0])
        q = (0.5 * atm[:, 2]) * (vn * vn)
        w, x, y, zz = r[:, 7], r[:, 8], r[:, 9], r[:, 10]
        nrm = np.sqrt(((w * w + x * x) + y * y) + zz * zz)
        quat_dev = np.abs(nrm - 1.0)
        unit = nrm > 1e-12
        safe = np.where(unit, nrm, 1.0)
        w, x, y, zz = (np.where(unit, w / safe, 1.0), np.where(unit, x / safe, 0.0), np.where(unit, y / safe, 0.0),
                       np.where(unit, zz / safe, 0.0))
        R = [[1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y)],
             [2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - w * x)],
             [2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)]]
        vb = [(R[0][i] * vr[:, 0] + R[1][i] * vr[:, 1]) + R[2][i] * vr[:, 2] for i in range(3)]
        alpha_total = np.arctan2(np.sqrt(vb[1] * vb[1] + vb[2] * vb[2]), vb[0])
        accel = (diag[:, 8] - diag[:, 9]) / diag[:, 4]
        margin = diag[:, 14]
        omega = np.max(np.abs(r[:, 11:14]), axis=1)
        env[E.ENV_MAX_Q], iq = first_best(q, ascent)
        if iq >= 0:
            env[E.ENV_MAX_Q_TIME], env[E.ENV_MAX_Q_ALT], env[E.ENV_MAX_Q_MACH] = ts[iq], z[iq], mach[iq]
        env[E.ENV_MAX_MACH] = first_best(mach, ascent)[0]
        env[E.ENV_MAX_Q_ALPHA] = first_best(q * alpha_total, ascent)[0]
        env[E.ENV_MAX_AXIAL_ACCEL] = first_best(accel, ascent)[0]
        env[E.ENV_MIN_STABILITY] = first_best(margin, ascent, largest=False)[0]
        env[E.ENV_MAX_OMEGA] = first_best(omega, every)[0]
        env[E.ENV_MAX_QUAT_DEV] = first_best(quat_dev, every)[0]
        if b >= 0:
            env[E.ENV_BURNOUT_TIME], env[E.ENV_BURNOUT_ALT] = ts[b], z[b]
            env[E.ENV_BURNOUT_SPEED] = np.sqrt((r[b, 4] * r[b, 4] + r[b, 5] * r[b, 5]) + r[b, 6] * r[b, 6])
            env[E.ENV_BURNOUT_STABILITY] = margin[b]
    return env, {"ts": ts, "z": z, "q": q, "mach": mach, "b": b, "a": a, "iq": iq, "ascent": ascent}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def close(got, exp):
    if np.isnan(exp) or np.isnan(got):
        return bool(np.isnan(exp) and np.isnan(got))
    return abs(got - exp) <= TOL * max(abs(exp), 1e-300)


def check_column(got, exp, per, tag):
    """One envelope column against its restatement, under the bounds of the module docstring."""
    print(tag, "got", [float(v) for v in got])
    print(tag, "exp", [float(v) for v in exp])
    for row in EXACT_ROWS:
        assert same_bits(got[row], exp[row]), (tag, analysis.ENVELOPE_NAMES[row], got[row], exp[row])
    for row in VALUE_ROWS:
        assert close(got[row], exp[row]), (tag, analysis.ENVELOPE_NAMES[row], got[row], exp[row])
    max_q_rows = (E.ENV_MAX_Q_TIME, E.ENV_MAX_Q_ALT, E.ENV_MAX_Q_MACH)
    if per is None or per["iq"] < 0:
        assert all(np.isnan(got[row]) for row in max_q_rows), tag
        return
    hit = np.nonzero(per["ts"] == got[E.ENV_MAX_Q_TIME])[0]
    assert len(hit) == 1 and per["ascent"][hit[0]], (tag, got[E.ENV_MAX_Q_TIME])
    g = int(hit[0])
    assert close(per["q"][g], exp[E.ENV_MAX_Q]), (tag, g, per["iq"])       # the oracle's q at the record the GPU chose
    assert got[E.ENV_MAX_Q_ALT] == per["z"][g] and close(got[E.ENV_MAX_Q_MACH], per["mach"][g]), (tag, g)


def envelope_of(engine, db, ids, records):
    """engine.flight_envelope on hand-made captures: records = list of [len_j, 15] arrays -> [16, m] NumPy."""
    m, cap = len(records), max(1, max(len(r) for r in records))
    traj = np.full((m, cap, 15), NAN)
    for j, r in enumerate(records):
        traj[j, :len(r)] = r
    tlen = np.array([len(r) for r in records], dtype=np.int64)
    dev = engine.device
    out = engine.flight_envelope(db, torch.as_tensor(np.asarray(ids, dtype=np.int64), device=dev), torch.as_tensor(traj, device=dev),
                                 torch.as_tensor(tlen, device=dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the captures
class Flights:
    """One capturing run and its envelope, shared by the tests that read it (never modified)."""

    def __init__(self, engine, kind, planar, prec, stride, cap):
        from erpl_monte_carlo_sim_amd.engine import DeviceBatch
        self.kind, self.hb, self.cfg = kind, mc_batch(kind, 8, planar), H.make_config(kind)
        engine.set_config(self.cfg)
        self.db = DeviceBatch.from_host(self.hb, engine.device, prec)
        self.summ, self.status, self.traj, self.tlen = engine.run(self.db, traj_ids=list(range(8)), traj_stride=stride, traj_cap=cap)
        self.ids = engine._keep
        self.env_dev = engine.flight_envelope(self.db, self.ids, self.traj, self.tlen)
        torch.cuda.synchronize()
        self.env, self.rec, self.len = self.env_dev.cpu().numpy(), self.traj.cpu().numpy(), self.tlen.cpu().numpy()
        self.rail = self.summ[_abi.SUM_RAIL_EXIT_TIME].cpu().numpy()

    def records(self, j):
        return self.rec[j, :int(self.len[j])]


@pytest.fixture(scope="module")
def liquid(engine):
    return Flights(engine, "liquid", True, _abi.PREC_F64, 25, 2000)


@pytest.fixture(scope="module")
def liquid_expected(liquid, oracle):
    return [restate(oracle, liquid.cfg, liquid.hb.take([j]), liquid.records(j)) for j in range(8)]


def test_real_flights_against_the_restatement(engine, oracle, liquid, liquid_expected):
    f = liquid
    assert f.env.shape == (16, 8)
    blown = 0
    for j in range(8):
        rec = f.records(j)
        assert rec[0, 0] == f.rail[j]            # record 0 carries the rail-exit time: the kernel needs no summary
        exp, per = liquid_expected[j]
        check_column(f.env[:, j], exp, per, f"liquid[{j}]")
        assert per["b"] >= 0 and per["a"] > per["iq"] > 0 and exp[E.ENV_USABLE] == len(rec) > per["a"] + 1
        with np.errstate(all="ignore"):
            blown += bool(np.max(np.abs(rec[:, 4:7])) > 1e30)
        assert np.isfinite(f.env[:14, j]).all()
    assert blown >= 1                            # the finite-only rule and the ascent window are both exercised


def test_exact_rows_on_blow_ups(engine, oracle):
    f = Flights(engine, "solid", False, _abi.PREC_F64_FAST, 7, 1500)
    for j in range(8):
        exp, per = restate(oracle, f.cfg, f.hb.take([j]), f.records(j))
        got = f.env[:, j]
        print(f"solid[{j}] len", int(f.len[j]), "got", [float(v) for v in got])
        for row in (E.ENV_USABLE, E.ENV_APOGEE_RECORD, E.ENV_MAX_OMEGA, E.ENV_MAX_QUAT_DEV, E.ENV_BURNOUT_TIME, E.ENV_BURNOUT_ALT,
                    E.ENV_BURNOUT_SPEED, E.ENV_BURNOUT_STABILITY):
            assert same_bits(got[row], exp[row]), (j, analysis.ENVELOPE_NAMES[row], got[row], exp[row])
        assert per["b"] < 0 and np.isnan(got[E.ENV_BURNOUT_TIME:E.ENV_BURNOUT_STABILITY + 1]).all()
        assert not np.isinf(got).any()
        assert got[E.ENV_USABLE] == f.len[j] > 256


def test_hand_made_captures(engine, oracle, liquid, liquid_expected):
    f = liquid
    engine.set_config(f.cfg)   # (the engine is shared: another test may have configured it for its own motor)
    src = next(j for j in range(8) if f.len[j] >= 600 and liquid_expected[j][1]["a"] >= 400)
    base = f.records(src).copy()
    a0, b0 = liquid_expected[src][1]["a"], liquid_expected[src][1]["b"]
    assert 300 < a0 and 0 < b0 < a0
    cases = []   # (sample id, records, note)

    def case(sid, rec, note):
        cases.append((sid, np.array(rec, dtype=np.float64).reshape(-1, 15), note))

    def planted(r, c, v):
        rec = base.copy()
        rec[r, c] = v
        return rec

    for k, n in enumerate((0, 1, 255, 256, 257, 513)):
        case((5, 0, 5, 3, 5, 0)[k], base[:n], f"len {n}")
    case(5, planted(0, 9, NAN), "NaN in record 0")
    case(3, planted(300, 4, NAN), "NaN in record 300")
    case(5, planted(300, 0, NAN), "NaN time in record 300")
    case(0, planted(60, 5, np.inf), "inf velocity inside the ascent")
    case(7, planted(60, 5, -np.inf), "-inf velocity inside the ascent")
    case(3, base[:b0 - 10], "cut before burnout")
    # a tie in q: the STATE of the max-q record (q does not read the time) at a later record of the ascent, which keeps its
    # own time stamp - so MAX_Q_TIME tells which of the two was reported
    tie_id = 5
    _, per = restate(oracle, f.cfg, f.hb.take([tie_id]), base)
    iq, later = per["iq"], per["iq"] + 150
    assert 0 < iq and later < per["a"]
    tie = base.copy()
    tie[later, 1:] = tie[iq, 1:]
    case(tie_id, tie, "max-q tie")
    # two records share the largest altitude: the first one is the apogee
    twin = base.copy()
    twin[a0 + 2, 3] = twin[a0, 3]
    case(3, twin, "apogee tie")
    ids = [c[0] for c in cases]
    assert len(set(ids)) < len(ids) and ids != sorted(ids) and len(ids) != f.hb.n
    got = envelope_of(engine, f.db, ids, [c[1] for c in cases])
    for j, (sid, rec, note) in enumerate(cases):
        exp, p = restate(oracle, f.cfg, f.hb.take([sid]), rec)
        check_column(got[:, j], exp, p, note)
    by_note = {c[2]: got[:, j] for j, c in enumerate(cases)}
    assert by_note["len 0"][E.ENV_USABLE] == 0 and np.isnan(by_note["len 0"][:15]).all()
    assert by_note["NaN in record 0"][E.ENV_USABLE] == 0 and np.isnan(by_note["NaN in record 0"][:15]).all()
    assert by_note["len 1"][E.ENV_USABLE] == 1 and by_note["len 1"][E.ENV_APOGEE_RECORD] == 0
    assert by_note["len 1"][E.ENV_MAX_Q_TIME] == 0.0 and np.isfinite(by_note["len 1"][E.ENV_MAX_Q])
    assert by_note["NaN in record 300"][E.ENV_USABLE] == 300 and by_note["NaN time in record 300"][E.ENV_USABLE] == 300
    assert by_note["inf velocity inside the ascent"][E.ENV_USABLE] == 60
    assert np.isnan(by_note["cut before burnout"][E.ENV_BURNOUT_TIME]) and by_note["cut before burnout"][E.ENV_USABLE] == b0 - 10
    assert by_note["max-q tie"][E.ENV_MAX_Q_TIME] == base[iq, 0] - base[0, 0]
    assert by_note["apogee tie"][E.ENV_APOGEE_RECORD] == a0


def test_columns_are_independent_and_repeatable(engine, liquid):
    f = liquid
    engine.set_config(f.cfg)
    again = engine.flight_envelope(f.db, f.ids, f.traj, f.tlen)
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int64), f.env_dev.view(torch.int64))
    for j in (0, 3, 7):
        alone = engine.flight_envelope(f.db, f.ids[j:j + 1].contiguous(), f.traj[j:j + 1].contiguous(), f.tlen[j:j + 1].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(alone[:, 0].view(torch.int64), f.env_dev[:, j].view(torch.int64)), j
    empty = engine.flight_envelope(f.db, f.ids[:0].contiguous(), f.traj[:0].contiguous(), f.tlen[:0].contiguous())
    assert tuple(empty.shape) == (16, 0)


def test_one_definition_with_extract_histories(engine, liquid, liquid_expected):
    """The envelope kernel and erpl_mc_extract_histories call ONE per-record evaluation: bit for bit the same values."""
    f = liquid
    engine.set_config(f.cfg)
    for j in range(8):
        per = liquid_expected[j][1]
        u, a, b = int(f.env[E.ENV_USABLE, j]), per["a"], per["b"]
        hist = engine.extract_histories(f.db, j, f.traj[j, :u], float(f.rec[j, 0, 0])).cpu().numpy()
        with np.errstate(all="ignore"):
            accel = (hist[:, 8] - hist[:, 9]) / hist[:, 4]
        assert same_bits(f.env[E.ENV_MIN_STABILITY, j], first_best(hist[:, 14], per["ascent"], largest=False)[0]), j
        assert same_bits(f.env[E.ENV_BURNOUT_STABILITY, j], hist[b, 14]), j
        assert same_bits(f.env[E.ENV_MAX_AXIAL_ACCEL, j], first_best(accel, per["ascent"])[0]), j
        assert a == int(f.env[E.ENV_APOGEE_RECORD, j])


def test_fp32_batch_is_refused(engine, liquid):
    from erpl_monte_carlo_sim_amd.engine import DeviceBatch
    db32 = DeviceBatch.from_host(liquid.hb, engine.device, _abi.PREC_F32)
    with pytest.raises(_abi.ErplError, match=r"rc=-1.*precision"):
        engine.flight_envelope(db32, liquid.ids, liquid.traj, liquid.tlen)


def test_python_layer():
    from erpl_monte_carlo_sim_amd import sampling
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    from erpl_monte_carlo_sim_amd.simulator import shared_engine
    mc = MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)
    out = mc.flight_envelope(dict(H.EXAMPLE_IC), 64, stride=25, seed=5, planar=True)
    ref = mc.run_monte_carlo_device(dict(H.EXAMPLE_IC), 64, seed=5, planar=True)
    # capturing changes no summary (a NaN equals a NaN, as everywhere the suite compares summaries: the capture
    # instantiation need not give a NaN the sign and payload the plain launch gives it)
    assert bool(((out["summary"] == ref["summary"]) | (out["summary"].isnan() & ref["summary"].isnan())).all())
    assert torch.equal(out["status"], ref["status"])
    env = out["envelope"]
    assert tuple(env.shape) == (16, 64) and env.dtype == torch.float64 and env.is_cuda
    assert out["envelope_names"] == list(analysis.ENVELOPE_NAMES) and tuple(out["reasons"].shape) == (64,)
    assert out["performance"]["sub_batches"] == 1
    q_alt, apogee = env[_abi.ENV_MAX_Q_ALT], out["summary"][_abi.SUM_FIRST_APOGEE_ALT]
    both = torch.isfinite(q_alt) & torch.isfinite(apogee)
    assert bool(both.any()) and bool((q_alt[both] <= apogee[both]).all())
    eng = shared_engine(None)
    assert H.same_nested(out["statistics"], analysis.envelope_statistics(env, out["reasons"], engine=eng))
    assert set(out["statistics"]) == set(analysis.ENVELOPE_NAMES)
    assert out["statistics"]["max_q"]["count"] == out["n_samples"] > 0
    # three sub-batches: 24 + 24 + 16 samples, each drawn from its own seed and reduced from its own capture
    cap = out["performance"]["records_per_sample"]
    assert cap == int(np.ceil(mc.max_time / 0.005 / 25)) + 4
    split = mc.flight_envelope(dict(H.EXAMPLE_IC), 64, stride=25, seed=5, planar=True, capture_bytes=24 * cap * 120 + 119)
    assert split["performance"]["sub_batches"] == 3 and tuple(split["envelope"].shape) == (16, 64)
    eng.set_config(mc._config())
    for j, (lo, nb) in enumerate(((0, 24), (24, 24), (48, 16))):
        db = sampling.synthetic_dispersions(nb, mc.rocket, mc.motor, mc.wind_model, dict(H.EXAMPLE_IC), eng.device,
                                            precision=_abi.PREC_F64_FAST, seed=5 + 1000003 * j, uncertainty=mc.uncertainty_params,
                                            base_altitude_profile=None, base_wind_profile=None, planar=True, engine=eng)
        summ, status, traj, tlen = eng.run(db, traj_ids=np.arange(nb), traj_stride=25, traj_cap=cap)
        part = eng.flight_envelope(db, eng._keep, traj, tlen)
        torch.cuda.synchronize()
        assert torch.equal(part.view(torch.int64), split["envelope"][:, lo:lo + nb].contiguous().view(torch.int64)), j
        assert torch.equal(summ.view(torch.int64), split["summary"][:, lo:lo + nb].contiguous().view(torch.int64)), j
