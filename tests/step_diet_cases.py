"""The batches and the calls behind tests/golden/step_diet_bits_*.npy: what test_gpu_step_diet_bits.py compares and what
tools/record_step_diet_bits.py records (no reference access).

The fp64 throughput RHS has two branches a wave skips as a whole when no lane needs them: the parachute drag and the
aerodynamic forces (`!chute && qdyn > 0`).  A change to how the force and moment sums are initialised around them can only go
wrong in a wave that holds lanes on BOTH sides of a branch in the same evaluation, so every group of 64 consecutive samples
here - the lanes of one wave: a fresh batch is popped in runs of 64 - mixes, from the first step on:

    parachute out / not out     thrust x 0.25 .. 0.28 is back below 500 m within seconds, the rest of the wave still climbs
    q_dynamic > 0 / == 0        one sample leaves no rail (burn time 0), stands still and has an all-zero wind table: at rest
                                relative to the wind in the first evaluation of its first step
    burning / burnt out         burn time x 0.2 .. 0.5 beside the full burn
    finite / non-finite         four samples of the reference's own 3-D dispersion model: they tumble, pass the hand-over
                                speed and turn non-finite
    every end of a flight       landing with and without the parachute, the altitude limit, a coast time-out, max_time

The steered samples are the one Set P sample of flight_event_cases.py with its steerings; the tumbling ones come from
flatten.dispersed_batch without `planar`.  192 samples are the 64 at three masses."""
import functools

import numpy as np
import torch

from erpl_monte_carlo_sim_amd import _abi, flatten, models
from erpl_monte_carlo_sim_amd.engine import DeviceBatch

import flight_event_cases as events
import helpers as H

SIZES = (64, 192)
MODES = ("run", "submit")
N_TUMBLE = 4
REST = 7                       # the lane of the sample at rest
# (thrust x, burn time x) of the steered lanes: the classes of flight_event_cases.py, then a ladder of thrusts
STEER = (events._STEP1[:2] + events._LOW + events._CHUTE + events._T(0.9, 1.0, 1.1, 1.2) + events._HIGH + events._OUT
         + events._T(*np.linspace(0.3, 1.7, 64 - 24 - N_TUMBLE - 1).tolist()))
assert len(STEER) + N_TUMBLE + 1 == 64


def config():
    return H.make_config("liquid")


@functools.lru_cache(maxsize=None)
def _wave():
    """The 64 samples of one wave, at the nominal mass."""
    base = events._base("liquid")
    pl = flatten.generate_parameter_samples(H.UNCERTAINTY, N_TUMBLE)
    tumble = flatten.dispersed_batch(models.Rocket(), H.make_motor("liquid"), models.WindModel(), H.EXAMPLE_IC, pl, H.CSV_ALT,
                                     H.CSV_WIND)
    assert np.array_equal(tumble.alt_grid, base.alt_grid)
    hb = base.take([0] * 64)
    steered = [i for i in range(64 - N_TUMBLE) if i != REST]
    hb.motor[0, steered] *= np.array([s[0] for s in STEER])
    hb.motor[3, steered] *= np.array([s[1] for s in STEER])
    hb.motor[3, REST] = 0.0            # the rail loop is never entered: the flight starts from the initial conditions
    hb.ic[3:6, REST] = 0.0
    hb.ic[10:13, REST] = 0.0
    hb.wind[:, :, REST] = 0.0
    for k in range(N_TUMBLE):
        j = 64 - N_TUMBLE + k
        hb.ic[:, j], hb.rocket[:, j], hb.motor[:, j], hb.wind[:, :, j] = tumble.ic[:, k], tumble.rocket[:, k], tumble.motor[:, k], tumble.wind[:, :, k]
    return hb


@functools.lru_cache(maxsize=None)
def batch(n):
    """-> HostBatch of n = 64 or 192 samples: treat it as read-only."""
    assert n in SIZES
    w = _wave()
    hb = w.take(list(range(64)) * (n // 64))
    hb.rocket *= np.repeat(np.array(events.MASSES[:n // 64]), 64)[None, :]
    return hb


def collect(engine, n, mode):
    """Fly batch(n) with the fp64 throughput build through erpl_mc_run_batch (`run`) or as a submitted batch -> the
    [17, n] float64 array of a recording: the summary with the status words as a 17th row."""
    engine.set_config(config())
    db = DeviceBatch.from_host(batch(n), engine.device, _abi.PREC_F64_FAST)
    if mode == "submit":
        summ, status = engine.submit(db)
        engine.wait()
    else:
        summ, status = engine.run(db)
    torch.cuda.synchronize(engine.device)
    engine.synchronize()
    return np.concatenate([summ.cpu().numpy(), status.cpu().numpy().astype(np.float64)[None, :]])


def encode(flight):
    """[17, n] -> [2, 17, n] of finite numbers: the values with 0 where they are not finite, and 1 / 2 / 3 where they are
    NaN / +inf / -inf (the encoding of bench.py --dump-outputs)."""
    marker = np.select([np.isnan(flight), flight == np.inf, flight == -np.inf], [1.0, 2.0, 3.0], 0.0)
    return np.stack([np.where(marker == 0, flight, 0.0), marker])


def missing(flight):
    """What a recording must contain to be worth comparing against, per wave of 64 -> the names that are absent."""
    st = flight[16].astype(np.int64)
    end = st & 0xFF
    out = []
    for w in range(flight.shape[1] // 64):
        s = slice(64 * w, 64 * w + 64)
        chute = (st[s] & _abi.ST_CHUTE) != 0
        want = {
            "parachute out": chute.any(), "parachute not out": (~chute).any(),
            "ST_NAN": np.any(st[s] & _abi.ST_NAN), "finite": np.any((st[s] & _abi.ST_NAN) == 0),
            "hand-over speed": np.any(flight[_abi.SUM_MAX_SPEED, s] > 1e6),
            "END_GROUND": np.any(end[s] == _abi.END_GROUND), "END_ALTITUDE": np.any(end[s] == _abi.END_ALTITUDE),
            "END_COAST": np.any(end[s] == _abi.END_COAST), "END_MAX_TIME": np.any(end[s] == _abi.END_MAX_TIME),
            "complete": not np.any(st[s] & _abi.ST_INCOMPLETE),
            "the sample at rest flew": flight[_abi.SUM_STEPS, 64 * w + REST] > 1,
        }
        out += ["wave %d: %s" % (w, k) for k, ok in want.items() if not ok]
    return out


def file_name(n):
    """One recording per size: erpl_mc_run_batch and a submitted batch return the same bytes (the recorder checks it)."""
    return "step_diet_bits_%d.npy" % n
