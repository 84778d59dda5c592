"""Submitted batches in a process with the HIP default of four hardware queues (GPU_MAX_HW_QUEUES=4): three lanes of one
stream each, no sweep streams.  There the sweep launches of lane adoption and the hand-over sweep of the fp64 throughput
build follow the main launch on the lane's own stream, and the hand-over sweep runs the instantiation capped at 256
registers (note [3] of erpl_k_config.h).  None of it may change a bit.

Every case runs its four-queue work in ONE fresh child process (the runtime reads the variable once, when it starts) that
loads the inputs this process wrote and writes its outputs as .npy; this process - 24 queues (conftest.py): the
512-register sweep, adoption on second streams - computes the same batches with erpl_mc_run_batch (no adoption) and
compares bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi, models, sampling

import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD_HEAD = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch
from erpl_monte_carlo_sim_amd import _abi
from erpl_monte_carlo_sim_amd.engine import DeviceBatch, TrajectoryEngine
import helpers as H
assert os.environ["GPU_MAX_HW_QUEUES"] == "4"
D = %(dir)r
dev = torch.device("cuda", 0)
def load(i, prec):
    t = lambda name: torch.as_tensor(np.load(os.path.join(D, "in%%d_%%s.npy" %% (i, name))), device=dev)
    return DeviceBatch(t("ic"), t("rocket"), t("motor"), t("alt_grid"), t("wind"), prec)
def save(name, x):
    np.save(os.path.join(D, name + ".npy"), x.cpu().numpy())
eng = TrajectoryEngine(dev)
eng.set_config(H.make_config("liquid"))
assert eng.get_overlap() == 3
"""

_CHILD_TAIL = r"""
eng.synchronize()                        # raises on a lane hand-over that timed out
assert eng.get_overlap() == 3
dc = eng.debug_counters()
assert dc[3] == 0 and dc[4] == 4, dc     # nothing lost; the library sized itself for four queues ...
assert dc[5] <= 3, dc                    # ... and created a stream per lane, nothing else (the caller's is the fourth)
eng.close()
print("ok")
"""

# more batches than lanes, every slot reused
_SUBMIT_ALL = r"""
prec = %(prec)d
dbs = [load(i, prec) for i in range(%(k)d)]
outs = [eng.submit(db) for db in dbs]
eng.wait()
torch.cuda.synchronize()
for i, (s, t) in enumerate(outs):
    save("summary%%d" %% i, s)
    save("status%%d" %% i, t)
"""

# one batch twice: without lane adoption and with the library's default
_ADOPT_OR_NOT = r"""
db = load(0, %(prec)d)
iters = {}
for name, lanes in (("off", 0), ("default", -1)):
    eng.set_adopt(lanes)
    s, t = eng.submit(db)
    eng.wait()
    torch.cuda.synchronize()
    steps, iters[name] = eng.ticket_stats(eng.last_ticket)
    save("summary_" + name, s)
    save("status_" + name, t)
# the thin tails are handed over, not dropped and not flown twice: never more wave iterations than without (integers)
assert iters["default"] <= iters["off"], iters
print("wave iterations", iters)
"""

# trajectory capture behind two plain batches that keep the other lanes busy
_CAPTURE = r"""
db = load(0, %(prec)d)
keep = [eng.submit(db), eng.submit(db)]  # (their outputs stay allocated until they have been written)
s, t, traj, tlen = eng.submit(db, traj_ids=%(ids)r, traj_stride=%(stride)d, traj_cap=%(cap)d)
dc = eng.debug_counters()                # (of the capture batch: the most recent one)
assert dc[6] == 0 and dc[7] == 1, dc     # no adoption with capture; the hand-over sweep is the uncapped instantiation
eng.wait()
torch.cuda.synchronize()
save("summary0", s)
save("status0", t)
save("traj", traj)
save("traj_len", tlen)
"""


def run_child(tmp_path, body, **fmt):
    code = (_CHILD_HEAD + body + _CHILD_TAIL) % dict(fmt, root=ROOT, dir=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GPU_MAX_HW_QUEUES="4"))
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
    return r.stdout


@pytest.fixture(scope="module")
def engine():
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = TrajectoryEngine(torch.device("cuda", 0))
    eng.set_config(H.make_config("liquid"))
    yield eng
    eng.close()


def make_batches(engine, tmp_path, precision, sizes):
    """Set S dispersions, K = 100 synthetic wind, liquid motor (these blow up: the hand-over path runs); the inputs go to
    tmp_path for the child."""
    prec = _abi.PRECISIONS[precision]
    rocket, motor, wm = models.Rocket(), models.LiquidMotor(), models.WindModel()
    dbs = []
    for i, n in enumerate(sizes):
        db = sampling.synthetic_dispersions(n, rocket, motor, wm, H.EXAMPLE_IC, engine.device, precision=prec, seed=400 + i,
                                            uncertainty=H.UNCERTAINTY, n_wind_knots=100, engine=engine)
        for name in ("ic", "rocket", "motor", "alt_grid", "wind"):
            np.save(tmp_path / ("in%d_%s.npy" % (i, name)), getattr(db, name).cpu().numpy())
        dbs.append(db)
    return prec, dbs


def reference(engine, db, **kw):
    out = engine.run(db, **kw)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def assert_same(tmp_path, tag, ref_s, ref_t):
    s, t = np.load(tmp_path / ("summary%s.npy" % tag)), np.load(tmp_path / ("status%s.npy" % tag))
    assert np.array_equal(t, ref_t), tag
    assert np.array_equal(s, ref_s, equal_nan=True), tag


@pytest.mark.parametrize("precision,sizes", [("f64_fast", (4099, 64, 37, 4096, 4099, 1, 8192)), ("f32", (4099, 64, 8192))])
def test_submitted_batches_at_four_queues_equal_serial_runs(engine, tmp_path, precision, sizes):
    """Batches submitted back to back at four queues - sizes that are no multiple of a wave, less than a wave, one
    sample - give the bits of erpl_mc_run_batch for each of them, and no hand-over is lost."""
    prec, dbs = make_batches(engine, tmp_path, precision, sizes)
    run_child(tmp_path, _SUBMIT_ALL, prec=prec, k=len(dbs))
    for i, db in enumerate(dbs):
        ref_s, ref_t = reference(engine, db)
        assert_same(tmp_path, str(i), ref_s, ref_t)


def test_lane_adoption_on_the_lanes_own_stream(engine, tmp_path):
    """One batch submitted with lane adoption off and with the library's default: identical bits, equal to
    erpl_mc_run_batch, and (in the child) not more wave iterations with the default than without."""
    prec, (db,) = make_batches(engine, tmp_path, "f64_fast", (4099,))
    print(run_child(tmp_path, _ADOPT_OR_NOT, prec=prec))
    ref_s, ref_t = reference(engine, db)
    assert_same(tmp_path, "_off", ref_s, ref_t)
    assert_same(tmp_path, "_default", ref_s, ref_t)


def test_trajectory_capture_at_four_queues(engine, tmp_path):
    """Capture of three samples through erpl_mc_submit_batch at four queues: the records of this process's capture - exact
    time stamps, the same position columns - through the uncapped hand-over sweep (the child checks which one ran)."""
    prec, (db,) = make_batches(engine, tmp_path, "f64_fast", (1000,))
    ids, stride, cap = [0, 1, 2], 20, 3100
    run_child(tmp_path, _CAPTURE, prec=prec, ids=ids, stride=stride, cap=cap)
    ref_s, ref_t, ref_traj, ref_len = reference(engine, db, traj_ids=ids, traj_stride=stride, traj_cap=cap)
    assert_same(tmp_path, "0", ref_s, ref_t)
    traj, tlen = np.load(tmp_path / "traj.npy"), np.load(tmp_path / "traj_len.npy")
    assert np.array_equal(tlen, ref_len) and np.all(ref_len > 0)
    for m in range(len(ids)):
        k = int(min(ref_len[m], cap))
        assert np.array_equal(traj[m, :k, 0], ref_traj[m, :k, 0]), m                       # time stamps
        assert np.array_equal(traj[m, :k, 1:4], ref_traj[m, :k, 1:4], equal_nan=True), m   # position
