"""The batches and the calls behind tests/golden/flight_bits_*.npy: what test_gpu_flight_bits.py compares and what
tools/record_flight_bits.py records.  Only sampling.synthetic_dispersions, DeviceBatch.from_host (the `events` case, whose
steered batches flight_event_cases.py builds on the host) and TrajectoryEngine.run are used, so the same code runs on any
build of the library.

Every case flies with the full termination logic (flags = 0).  A recording is one float64 array per case and build:
the [16, n] summary with the status words as a 17th row (int32 values are exact in float64); the capture case also keeps
the captured records and their counts.  The `events` case flies its groups one after the other, each with its own
configuration and flags, and keeps their columns side by side in the order of flight_event_cases.groups()."""
import numpy as np
import torch

from erpl_monte_carlo_sim_amd import _abi, models, sampling
from erpl_monte_carlo_sim_amd.engine import DeviceBatch

import flight_event_cases as events
import helpers as H

PRECISIONS = ("f64_fast", "f32", "f64")
SEED = 1234
# name: (motor, wind, samples).  The first four are the specialisations the launcher picks for the throughput builds
# (wind table or none x liquid or solid motor) on Set S dispersions: the benchmark's own, seed 1234, K = 100 synthetic wind.
CASES = {
    "wind_liquid": ("liquid", "syn", 256),
    "wind_solid": ("solid", "syn", 256),
    "still_liquid": ("liquid", "none", 256),
    "still_solid": ("solid", "none", 256),
    "csv_chute": ("liquid", "csv", 128),     # planar, CSV base wind K = 6, down to the ground under the parachute
    "capture": ("liquid", "syn", 256),       # the trajectory-capture build (switches read at run time)
    "events": ("liquid", "events", events.N_SAMPLES),   # steered: every way a flight ends, coast-outs of both limits included
}
SET_S = ("wind_liquid", "wind_solid", "still_liquid", "still_solid")
CAPTURE_IDS, CAPTURE_STRIDE, CAPTURE_CAP = [0, 85, 170, 255], 200, 320


def make_batch(engine, case, precision):
    """The DeviceBatch of a case in the working precision of a build (the draws are fp64 in every build)."""
    kind, wind, n = CASES[case]
    prec = _abi.PRECISIONS[precision]
    csv = wind == "csv"
    db = sampling.synthetic_dispersions(n, models.Rocket(), H.make_motor(kind), models.WindModel(), H.EXAMPLE_IC, engine.device,
                                        precision=prec, seed=SEED, planar=csv, base_altitude_profile=H.CSV_ALT if csv else None,
                                        base_wind_profile=H.CSV_WIND if csv else None, n_wind_knots=100, engine=engine)
    if wind == "none":
        db = DeviceBatch(db.ic, db.rocket, db.motor, None, None, prec)
    return db


def collect_events(engine, precision):
    """The `events` case: every group of flight_event_cases.py under its own configuration and flags."""
    cols = []
    for g in events.groups():
        engine.set_config(events.config(g.name))
        out = engine.run(DeviceBatch.from_host(g.hb, engine.device, _abi.PRECISIONS[precision]), flags=g.flags)
        torch.cuda.synchronize(engine.device)
        cols.append(np.concatenate([out[0].cpu().numpy(), out[1].cpu().numpy().astype(np.float64)[None, :]]))
    return {"flight": np.concatenate(cols, axis=1)}


def collect(engine, case, precision):
    """Fly a case with one build -> {name: float64 array}, the arrays a recording holds."""
    if case == "events":
        return collect_events(engine, precision)
    engine.set_config(H.make_config(CASES[case][0]))
    db = make_batch(engine, case, precision)
    kw = dict(traj_ids=CAPTURE_IDS, traj_stride=CAPTURE_STRIDE, traj_cap=CAPTURE_CAP) if case == "capture" else {}
    out = engine.run(db, **kw)
    torch.cuda.synchronize(engine.device)
    summ, status = out[0].cpu().numpy(), out[1].cpu().numpy()
    rec = {"flight": np.concatenate([summ, status.astype(np.float64)[None, :]])}
    if case == "capture":
        rec["traj"] = out[2].cpu().numpy().reshape(len(CAPTURE_IDS), -1)
        rec["traj_len"] = out[3].cpu().numpy().astype(np.float64)
    return rec


def status_of(flight):
    return flight[16].astype(np.int64)


def missing_ends(case, flight):
    """What a recording must contain to be worth comparing against: every way a Set S flight ends, the parachute in the
    parachute case, the coast time-out next to the three other end reasons in the steered case.  Returns the names that are
    absent."""
    st = status_of(flight)
    end = st & 0xFF
    want = {}
    if case in SET_S or case == "capture":
        want = {"END_GROUND": np.any(end == _abi.END_GROUND), "END_ALTITUDE": np.any(end == _abi.END_ALTITUDE),
                "END_MAX_TIME": np.any(end == _abi.END_MAX_TIME), "ST_NAN": np.any(st & _abi.ST_NAN)}
    if case == "csv_chute":
        want = {"ST_CHUTE": np.any(st & _abi.ST_CHUTE), "END_GROUND": np.any(end == _abi.END_GROUND)}
    if case == "events":
        want = {"END_COAST": np.any(end == _abi.END_COAST), "END_ALTITUDE": np.any(end == _abi.END_ALTITUDE),
                "END_GROUND": np.any(end == _abi.END_GROUND), "END_MAX_TIME": np.any(end == _abi.END_MAX_TIME)}
    return [k for k, ok in want.items() if not ok]


def file_name(case, precision, name):
    return "flight_bits_%s_%s%s.npy" % (case, precision, "" if name == "flight" else "_" + name)
