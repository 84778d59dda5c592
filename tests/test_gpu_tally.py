"""erpl_mc_tally_* on the device.  The state after erpl_mc_tally_add / _merge against the state of erpl_mc_tally_add_host /
_merge_host (the same header code on the host, itself held to the restatement tally_ref by test_tally_abi.py), byte for byte
on the int64 words - never device against itself alone; a tally of flown samples against the resident calls (erpl_mc_analyze,
_histogram, _histogram_xy, _impact_density); and the run: run_monte_carlo_tally against run_monte_carlo_device, its
independence of the sub-batch size, refly of the held extremes, two ranks on one GPU."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, analysis, models

import helpers as H
import tally_cases as TC
import tally_ref as R
from tally_cases import check_against_ref, host_tally

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def analyzer():
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    return MonteCarloAnalyzer(models.Rocket(), models.LiquidMotor(), models.StandardAtmosphere(), models.WindModel(), verbose=False)


def device_tally(engine, spec, pieces, state=None):
    """The device state after one erpl_mc_tally_add per (summary, status, first_id); the summaries sit in wider tensors
    (ld > n) full of values that would change every count if they were read."""
    if state is None:
        _, state = engine.tally_new(spec)
    for summary, status, first_id in pieces:
        n = summary.shape[1]
        wide = torch.full((16, n + 3), 1234.5, dtype=torch.float64, device=engine.device)
        wide[:, :n] = torch.from_numpy(summary).to(engine.device)
        st = None if status is None else torch.from_numpy(np.concatenate([status, np.zeros(2, np.int32)])).to(engine.device)
        engine.tally_add(spec, state, wide, st, first_id=first_id, n=n)
    return state


def words(state):
    torch.cuda.synchronize()
    return state.cpu().numpy()


CASES = [(n, dict(k=5)) for n in TC.SIZES] + \
        [(257, dict(k=0)), (257, dict(k=1)), (63, dict(k=64)), (1025, dict(k=64)),
         (1025, dict(bins=(1, 1024, 1024, 1, 1024), zones=False)),
         (1025, dict(grid=TC.BIG_GRID)),      # impacts inside and outside the LDS tile of the grid
         (4099, dict(k=64)),          # more candidates than a list holds: the extremes come from the scan of the row
         (140003, dict(k=16))]        # more columns than one sweep of the grid: the stride loop


@pytest.mark.parametrize("n,kw", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_device_state_equals_host_state(engine, n, kw):
    d = TC.spec_dict(**kw)
    spec = TC.library_spec(d)
    summary, status = TC.table(n, seed=n)
    want = host_tally(spec, [(summary, status, 10 ** 12)])
    got = words(device_tally(engine, spec, [(summary, status, 10 ** 12)]))
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:20]
    assert words(device_tally(engine, spec, [(summary, status, 10 ** 12)])).tobytes() == got.tobytes()
    if n <= 4099:
        check_against_ref(d, spec, got, R.tally(d, summary, status, 10 ** 12))


def test_an_all_outlier_window_and_a_window_without_status(engine):
    d = TC.spec_dict()
    spec = TC.library_spec(d)
    summary, status = TC.table(65, all_outliers=True)
    got = words(device_tally(engine, spec, [(summary, status, 0)]))
    assert got.tobytes() == host_tally(spec, [(summary, status, 0)]).tobytes() and not got[16:].any()
    summary, _ = TC.table(257)
    assert words(device_tally(engine, spec, [(summary, None, 5)])).tobytes() == host_tally(spec, [(summary, None, 5)]).tobytes()


def test_windows_in_any_split_and_order_give_the_bytes_of_one_host_add(engine):
    d = TC.spec_dict(k=64)
    spec = TC.library_spec(d)
    n = 6000
    summary, status = TC.table(n, seed=21)
    cols = lambda a, b: (np.ascontiguousarray(summary[:, a:b]), status[a:b].copy(), 77 + a)
    want = host_tally(spec, [cols(0, n)])
    cut = [0, 1, 64, 129, 700, 3000, n]      # the 2300- and 3000-column windows overflow their candidate lists, the later ones
    pieces = [cols(cut[p], cut[p + 1]) for p in range(6)]     # of a filled tally go through the admission threshold
    assert words(device_tally(engine, spec, pieces)).tobytes() == want.tobytes()
    assert words(device_tally(engine, spec, pieces[::-1])).tobytes() == want.tobytes()
    assert words(device_tally(engine, spec, [cols(i, i + 1) for i in range(40)])).tobytes() == host_tally(spec, [cols(0, 40)]).tobytes()
    check_against_ref(d, spec, want, R.tally(d, summary, status, 77))


def test_device_merge_equals_host_merge(engine):
    d = TC.spec_dict(k=64)
    spec = TC.library_spec(d)
    n = 1025
    summary, status = TC.table(n)
    cols = lambda a, b: (np.ascontiguousarray(summary[:, a:b]), status[a:b].copy(), 77 + a)
    cut = [0, 1, 64, 129, 700, n]
    host = [host_tally(spec, [cols(cut[p], cut[p + 1])]) for p in range(5)]
    dev = [torch.from_numpy(h).to(engine.device) for h in host]       # the device merges what the host tallied
    for dst, src in ((3, 4), (3, 1), (0, 2)):
        analysis.tally_merge_host(spec, host[dst], host[src])
        engine.tally_merge(spec, dev[dst], dev[src])
        assert words(dev[dst]).tobytes() == host[dst].tobytes(), (dst, src)
    _, tree = engine.tally_new(spec)
    engine.tally_merge(spec, tree, dev[3])
    engine.tally_merge(spec, tree, dev[0])
    assert words(tree).tobytes() == host_tally(spec, [cols(0, n)]).tobytes()
    # and of what the device tallied, merged the other way round
    a, b = device_tally(engine, spec, [cols(0, 700)]), device_tally(engine, spec, [cols(700, n)])
    engine.tally_merge(spec, b, a)
    assert words(b).tobytes() == words(tree).tobytes()


def test_result_on_the_device_is_the_host_finalisation(engine):
    d = TC.spec_dict()
    spec = TC.library_spec(d)
    summary, status = TC.table(1025)
    state = device_tally(engine, spec, [(summary, status, 3)])
    dev, host = engine.tally_result(spec, state), analysis.tally_result_host(spec, words(state))
    assert bytes(dev["result"]) == bytes(host["result"])
    assert np.array_equal(dev["hist_counts"], host["hist_counts"]) and np.array_equal(dev["grid_counts"], host["grid_counts"])
    status[7] |= _abi.ST_INCOMPLETE
    with pytest.raises(_abi.IncompleteBatch):
        engine.tally_result(spec, device_tally(engine, spec, [(summary, status, 3)]))
    with pytest.raises(ValueError):
        engine.tally_add(spec, state[:-1], torch.zeros((16, 4), dtype=torch.float64, device=engine.device))
    with pytest.raises(_abi.ErplError, match="bins"):
        bad = TC.library_spec(d)
        bad.bins[0] = 0
        engine.tally_new(bad)


# ------------------------------------------------------------------------------------------------ flown samples
@pytest.fixture(scope="module", params=["planar", "diverging"])
def flown(analyzer, request):
    """4096 flights of the engine: the planar set (nearly every sample valid) and the reference's own dispersion model, under
    which most samples tumble, blow up and are filtered (non-finite rows, every reason bit)."""
    return analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 4096, planar=request.param == "planar")


def test_tally_of_flown_samples_equals_the_resident_calls(engine, flown):
    """4096 flights: header and reason counts of erpl_mc_analyze, the counts of erpl_mc_histogram / _histogram_xy over the same
    fixed ranges, the zone counts of erpl_mc_impact_density, min / max, and mean / std to a relative 1e-12."""
    summ, status = flown["summary"].contiguous(), flown["status"].contiguous()
    rows = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME, _abi.SUM_MAX_SPEED]
    ana, why = engine.analyze(summ, status, rows=rows, reasons=True)
    assert ana.n_valid >= 50
    ranges = [(0.0, 80000.0), (0.0, 200000.0), (0.0, 600.0), (0.0, 2000.0)]
    zones = [np.array([[-2000.0, -2000.0], [3000.0, -1000.0], [1000.0, 4000.0]]),
             np.array([[0.0, 0.0], [50000.0, 0.0], [50000.0, 50000.0], [0.0, 50000.0]])]
    grid_ranges = ((-20000.0, 20000.0), (-15000.0, 25000.0))
    # a centre near the mean (to the metre, from the resident run) keeps the variance well conditioned
    spec = analysis.tally_spec(rows=rows, ranges=ranges, bins=[1000, 50, 7, 1024], centres=[float(round(ana.row[j].mean)) for j in range(4)],
                               k=16, grid_bins=(128, 256), grid_ranges=grid_ranges, zones=zones)
    _, state = engine.tally_new(spec)
    engine.tally_add(spec, state, summ, status, first_id=0)
    assert words(state).tobytes() == host_tally(spec, [(summ.cpu().numpy(), status.cpu().numpy(), 0)]).tobytes()
    got = engine.tally_result(spec, state)
    res = got["result"]
    assert (res.n, res.n_valid, res.n_outliers) == (ana.n, ana.n_valid, ana.n_outliers)
    assert list(res.reason_counts) == list(ana.reason_counts) and list(res.termination_counts) == list(ana.termination_counts)
    assert (res.n_status_nan, res.n_incomplete) == (ana.n_status_nan, ana.n_incomplete)
    _, counts, info = engine.histogram(summ, why, rows=rows, bins=[1000, 50, 7, 1024], ranges=ranges)
    for j in range(4):
        row, want = res.row[j], ana.row[j]
        assert np.array_equal(got["hist_counts"][j, :spec.bins[j]], counts[j]), j
        assert (row.count, row.below, row.above) == (want.count, info["below"][j], info["above"][j]), j
        assert (row.min, row.max) == (want.min, want.max), j
        print(f"row {rows[j]}: mean {row.mean!r} vs {want.mean!r}, std {row.std!r} vs {want.std!r}")
        assert abs(row.mean - want.mean) <= 1e-12 * abs(want.mean), j
        assert abs(row.std - want.std) <= 1e-12 * abs(want.std), j
    cells, _, _, info2 = engine.histogram2d(summ, why, _abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y, bins=(128, 256), ranges=grid_ranges)
    assert np.array_equal(got["grid_counts"], cells) and (res.grid_counted, res.grid_outside) == (info2["counted"], info2["outside"])
    dens = engine.impact_density(summ, why, nodes=(2, 2), levels=(), zones=zones)
    assert [z["inside"] for z in dens["zones"]] == list(res.zone_inside[:2]) and res.grid_counted == dens["count"]
    # The same rows with the DEFAULT mid-range centres, which run_monte_carlo_tally uses.  The sums stay exact, but
    # var = (sum_d2 - sum_d (sum_d / count)) / count subtracts two numbers of size var + delta^2, delta = centre - mean, each
    # with a few roundings of 2^-53: the relative error of var is at most 4 u (1 + delta^2 / var), that of std half of it,
    # that of mean = centre + sum_d / count at most 4 u (|delta| + |mean|) / |mean| - the bound include/erpl_mc.h states -
    # on top of the 1e-12 of erpl_mc_analyze's own two-pass values.
    far = analysis.tally_spec(rows=rows, ranges=ranges, bins=[1000, 50, 7, 1024], k=16)
    _, state = engine.tally_new(far)
    engine.tally_add(far, state, summ, status, first_id=0)
    far_res = engine.tally_result(far, state)["result"]
    u = 2.0 ** -53
    for j in range(4):
        row, want = far_res.row[j], ana.row[j]
        delta = far.centre[j] - want.mean
        amp = 1.0 + delta * delta / (want.std * want.std)
        print(f"row {rows[j]}, default centre {far.centre[j]}: std off by {abs(row.std - want.std) / want.std:.3g}, bound {2 * u * amp + 1e-12:.3g}")
        assert abs(row.std - want.std) <= (2 * u * amp + 1e-12) * want.std, j
        assert abs(row.mean - want.mean) <= 4 * u * (abs(delta) + abs(want.mean)) + 1e-12 * abs(want.mean), j


def states_of(analyzer, monkeypatch, chunk, **kw):
    monkeypatch.setattr(analyzer, "DEVICE_CHUNK", chunk)
    return analyzer.run_monte_carlo_tally(dict(H.EXAMPLE_IC), 1024, planar=True, **kw)


def test_a_tally_run_does_not_depend_on_the_sub_batches_and_equals_the_resident_run(engine, analyzer, monkeypatch):
    small = states_of(analyzer, monkeypatch, 128, design="lhs")
    large = states_of(analyzer, monkeypatch, 512, design="lhs")
    assert small["performance"]["sub_batches"] == 8 and large["performance"]["sub_batches"] == 2
    assert words(small["state"]).tobytes() == words(large["state"]).tobytes()
    resident = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 1024, planar=True, design="lhs")
    spec, state = engine.tally_new(small["spec"])
    engine.tally_add(spec, state, resident["summary"].contiguous(), resident["status"].contiguous(), first_id=0)
    assert words(state).tobytes() == words(small["state"]).tobytes()
    assert small["n_samples"] == resident["n_samples"] and small["design"] == resident["design"]
    assert small["rows"]["apogee_altitude"]["count"] == resident["n_samples"]
    # without a design the inputs depend on the sub-batch size: one size, against the resident run of that size
    plain = states_of(analyzer, monkeypatch, 512)
    resident = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 1024, planar=True)
    spec, state = engine.tally_new(plain["spec"])
    engine.tally_add(spec, state, resident["summary"].contiguous(), resident["status"].contiguous(), first_id=0)
    assert words(state).tobytes() == words(plain["state"]).tobytes()
    assert plain["design"] is None
    with pytest.raises(ValueError, match="design"):
        analyzer.refly(plain, [0])


def test_refly_flies_the_held_extremes_again(analyzer, monkeypatch):
    run = states_of(analyzer, monkeypatch, 256, design="lhs")
    resident = analyzer.run_monte_carlo_device(dict(H.EXAMPLE_IC), 1024, planar=True, design="lhs")
    worst = run["rows"]["range"]["largest"]
    ids = [i for _, i in worst]
    again = analyzer.refly(run, ids, stride=10)
    got = again["summary"].cpu().numpy()
    assert got.shape == (16, len(ids)) and len(ids) == 16
    assert got[_abi.SUM_RANGE].tobytes() == np.array([v for v, _ in worst]).tobytes()                 # to the bit
    assert np.array_equal(again["status"].cpu().numpy(), resident["status"].cpu().numpy()[ids])
    assert np.array_equal(got, resident["summary"].cpu().numpy()[:, ids], equal_nan=True)
    assert int(again["traj_len"].min()) > 0


_RANK_CODE = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch
import torch.distributed as td
td.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
import erpl_monte_carlo_sim_amd as E
import helpers as H
mc = E.MonteCarloAnalyzer(E.Rocket(), E.LiquidMotor(), E.StandardAtmosphere(), E.WindModel(), device="cuda:0", verbose=False)
mc.DEVICE_CHUNK = 100
out = mc.run_monte_carlo_tally(dict(H.EXAMPLE_IC), 601, planar=True, design="lhs")
torch.cuda.synchronize()
np.save(os.environ["ERPL_TEST_OUT"] + f".{td.get_rank()}.npy", out["state"].cpu().numpy())
td.barrier()
td.destroy_process_group()
"""


def test_two_ranks_merge_to_the_state_of_one(tmp_path, analyzer, monkeypatch):
    """Two FRESH processes on cuda:0 (gloo), 301 and 300 samples of one 601-column design in sub-batches of 100: one
    all-gather of the state words, merged in rank order - the state of a one-rank run, byte for byte, on both ranks."""
    out = str(tmp_path / "state")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2", ERPL_TEST_OUT=out,
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, "-c", _RANK_CODE % {"root": ROOT}], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    monkeypatch.setattr(analyzer, "DEVICE_CHUNK", 1 << 20)
    one = words(analyzer.run_monte_carlo_tally(dict(H.EXAMPLE_IC), 601, planar=True, design="lhs")["state"])
    for r in range(2):
        assert np.load(out + f".{r}.npy").tobytes() == one.tobytes(), r
