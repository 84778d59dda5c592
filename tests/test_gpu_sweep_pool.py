"""Sweep streams from the HIP runtime's other stream-priority pool (erpl_mc_set_sweep_pool) in a process with the HIP default
of four hardware queues: a lane's sweeps and hand-over sweep run on a second stream created with
hipStreamCreateWithPriority, the lane's next batch follows the main launch on a second workspace - the code paths every
24-queue test runs, selected by another condition.  None of it may change a bit.

As in test_gpu_four_queues.py (whose helpers this file imports), the four-queue work of a case runs in ONE fresh child
process with GPU_MAX_HW_QUEUES=4; this process (24 queues) computes the same batches with erpl_mc_run_batch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erpl_monte_carlo_sim_amd import _abi

from test_gpu_four_queues import ROOT, _CHILD_HEAD, assert_same, engine, make_batches, reference  # noqa: F401 (engine: fixture)

pytestmark = pytest.mark.gpu

THRESHOLD = 9216      # kSweepPoolMinBatch of erpl_plan.h: the automatic rule switches the pool on from this batch size

# two rounds over the same batches: the second one reuses every lane and both workspaces of each
_FORCED_ON = r"""
eng.set_sweep_pool(1)
prec = %(prec)d
dbs = [load(i, prec) for i in range(%(k)d)]
outs = [eng.submit(db) for db in dbs + dbs]
eng.wait()
torch.cuda.synchronize()
for i, (s, t) in enumerate(outs):
    save("summary%%d" %% i, s)
    save("status%%d" %% i, t)
eng.synchronize()                        # raises on a lane hand-over that timed out
dc = eng.debug_counters()
assert dc[3] == 0 and dc[4] == 4, dc     # nothing lost; the library still sizes itself for four queues
assert dc[5] == 6, dc                    # a main and a sweep stream per lane
assert dc[7] == 2 + 16 + 32, dc          # capped hand-over sweep, on the lane's second stream, which is from the other pool
assert dc[6] == 40, dc
assert eng.get_overlap() == 3
"""

# the automatic rule, then a second context that never uses the pool
_AUTOMATIC = r"""
prec = %(prec)d
small, large = load(0, prec), load(1, prec)
s, t = eng.submit(small)
eng.wait()
torch.cuda.synchronize()
dc = eng.debug_counters()
assert dc[5] <= 3 and not int(dc[7]) & 16, dc      # a few thousand samples: one stream per lane, as before
assert int(dc[7]) & 15 == 2, dc
before = dc[5]
save("summary0", s)
save("status0", t)
s, t = eng.submit(large)
eng.wait()
torch.cuda.synchronize()
dc = eng.debug_counters()
assert dc[5] == before + 2, dc                     # the next lane's main stream and its sweep stream
assert int(dc[7]) & 16 and int(dc[7]) & 32 and dc[6] == 40, dc
save("summary1", s)
save("status1", t)
eng.synchronize()
assert eng.debug_counters()[3] == 0 and eng.get_overlap() == 3

off = TrajectoryEngine(dev)
off.set_config(H.make_config("liquid"))
off.set_sweep_pool(0)
s, t = off.submit(large)
off.wait()
torch.cuda.synchronize()
dc = off.debug_counters()
assert dc[3] == 0 and dc[4] == 4 and dc[5] == 1 and dc[6] == 40 and dc[7] == 2, dc   # today's counters
save("summary2", s)
save("status2", t)
off.synchronize()
off.close()
"""

_TIME_OUT = r"""
db = load(0, %(prec)d)
eng.set_sweep_pool(1)
eng.set_adopt_spin(-1)
s, t = eng.submit(db)
ticket = eng.last_ticket
eng.wait(ticket)
torch.cuda.current_stream().synchronize()
n_lost = int(((t & _abi.ST_INCOMPLETE) != 0).sum())
dc = eng.debug_counters()
assert n_lost > 0 and dc[3] == n_lost, (n_lost, dc)
assert int(dc[7]) & 32, dc
for call in (lambda: eng.check(ticket), eng.synchronize):
    try:
        call()
    except _abi.IncompleteBatch:
        pass
    else:
        raise AssertionError("the injected time-out passed silently")
eng.set_adopt_spin(1 << 22)              # the knob back to its default: the same workspaces run clean again
outs = [eng.submit(db) for _ in range(6)]
eng.wait()
torch.cuda.synchronize()
eng.synchronize()
for i, (s, t) in enumerate(outs):
    save("summary%%d" %% i, s)
    save("status%%d" %% i, t)
"""

_TAIL = r"""
eng.close()
print("ok")
"""


def run_child(tmp_path, body, **fmt):
    code = (_CHILD_HEAD + body + _TAIL) % dict(fmt, root=ROOT, dir=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GPU_MAX_HW_QUEUES="4"))
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
    return r.stdout


def test_forced_pool_streams_equal_serial_runs(engine, tmp_path):
    """erpl_mc_set_sweep_pool(1) at four queues: batches of every awkward size, submitted back to back twice over, give the
    bits of erpl_mc_run_batch; the child checks the streams created and what word 7 reports."""
    sizes = (4099, 64, 37, 4096, 1, 8192)
    prec, dbs = make_batches(engine, tmp_path, "f64_fast", sizes)
    run_child(tmp_path, _FORCED_ON, prec=prec, k=len(dbs))
    for i, db in enumerate(dbs):
        ref_s, ref_t = reference(engine, db)
        assert_same(tmp_path, str(i), ref_s, ref_t)
        assert_same(tmp_path, str(i + len(dbs)), ref_s, ref_t)


def test_pool_streams_come_with_the_first_batch_that_fills_the_gpu(engine, tmp_path):
    """The default mode: a 4 099-sample batch keeps the lane on one stream, the following batch of THRESHOLD + 37 samples
    brings the pool streams; a context with erpl_mc_set_sweep_pool(0) runs that batch with the counters it had before.
    All three results are those of erpl_mc_run_batch."""
    prec, (small, large) = make_batches(engine, tmp_path, "f64_fast", (4099, THRESHOLD + 37))
    run_child(tmp_path, _AUTOMATIC, prec=prec)
    ref_s, ref_t = reference(engine, small)
    assert_same(tmp_path, "0", ref_s, ref_t)
    ref_s, ref_t = reference(engine, large)
    assert_same(tmp_path, "1", ref_s, ref_t)
    assert_same(tmp_path, "2", ref_s, ref_t)


def test_timed_out_hand_over_fails_the_batch_with_pool_streams(engine, tmp_path):
    """The injected hand-over time-out (erpl_mc_set_adopt_spin(-1): a record is lost by design, nothing faults) still
    fails the batch with ERPL_ERR_INCOMPLETE when its sweeps run on a pool stream, and the workspaces run clean after."""
    prec, (db,) = make_batches(engine, tmp_path, "f64_fast", (20000,))
    run_child(tmp_path, _TIME_OUT, prec=prec)
    ref_s, ref_t = reference(engine, db)
    for i in range(6):
        assert_same(tmp_path, str(i), ref_s, ref_t)


def test_setter_modes_and_a_process_without_use_for_the_pool(engine, tmp_path):
    """Every mode returns cleanly, anything else is refused; where the pool is not used (this process has a hardware queue
    per stream; a device with one stream priority takes the same early return) mode 1 behaves like mode 0."""
    prec, (db,) = make_batches(engine, tmp_path, "f64_fast", (4099,))
    ref_s, ref_t = reference(engine, db)
    try:
        for mode in (0, 1, -1, 1):
            engine.set_sweep_pool(mode)
        s, t = engine.submit(db)
        engine.wait()
        torch.cuda.synchronize()
        engine.synchronize()
        dc = engine.debug_counters()
        assert not int(dc[7]) & 32, dc
        assert np.array_equal(t.cpu().numpy(), ref_t) and np.array_equal(s.cpu().numpy(), ref_s, equal_nan=True)
        for bad in (2, -2):
            with pytest.raises(_abi.ErplError):
                engine.set_sweep_pool(bad)
    finally:
        engine.set_sweep_pool(-1)
