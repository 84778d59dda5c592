"""Shared helpers: golden-fixture loading and batch construction (no reference access)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from erpl_monte_carlo_sim_amd import _abi, flatten, models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = C.c_void_p(0x1000)      # stands in for a device pointer that an argument check never dereferences

EXAMPLE_IC = {
    "position": [0.0, 0.0, 10.0],
    "velocity": [0, 0, 0.0],
    "attitude": [0.0, -np.pi / 2 + 0.02, 0.0],
    "angular_velocity": [0.0, 0.0, 0.0],
}

CSV_ALT = np.array([0.0, 5000.0, 10000.0, 15000.0, 20000.0, 25000.0])
CSV_WIND = np.array([[2.0, 0, 0], [5, 1, 0], [8, 2, 0], [10, 2, 0], [12, 3, 0], [15, 3, 0]])

UNCERTAINTY = {
    "initial_position": [0.0, 0.0, 0.0], "initial_velocity": [0.1, 0.1, 0.1],
    "initial_attitude": [0.005, 0.005, 0.005], "initial_angular_velocity": [0.005, 0.005, 0.005],
    "mass_uncertainty": 0.02, "thrust_uncertainty": 0.03, "wind_speed_range": [0.0, 5.0],
    "wind_direction_range": [0.0, 2 * np.pi], "atmospheric_density_uncertainty": 0.05,
}


def load_lib():
    """The package's own library for the tests of the C boundary that need no GPU, built first if it is not there."""
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _abi.load_library()


def check_struct_layouts(tmp_path, structs, macros):
    """sizeof and the offset of EVERY field of the ctypes mirrors `structs` ((C name, _abi name), ..) and the values of
    `macros` ((C macro, value in _abi), ..) == what gcc sees in include/erpl_mc.h."""
    lines, want = [], []
    for cname, pyname in structs:
        cls = getattr(_abi, pyname)
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(cls))
        for field, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {field}));')
            want.append(getattr(cls, field).offset)
    for macro, val in tuple(macros) + (("ERPL_MC_ABI_VERSION", _abi.ABI_VERSION),):
        lines.append(f'printf("%d\\n", (int){macro});')
        want.append(val)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "erpl_mc.h"\nint main(){' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == want
    assert _abi.ABI_VERSION == 4


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


def load_flights(name):
    idx = load_json(name + ".json")
    arr = np.load(os.path.join(GOLDEN, name + ".npz"))
    return idx, arr


def make_motor(kind):
    return models.SolidMotor() if kind in ("solid", 1) else models.LiquidMotor()


def make_config(kind, **kw):
    return flatten.config_from_objects(models.Rocket(), make_motor(kind), models.StandardAtmosphere(), **kw)


def batch_from_golden(entries, arr):
    """HostBatch from golden flight entries that share motor kind and wind grid."""
    n = len(entries)
    e0 = entries[0]
    k = arr[e0["tag"] + "_altitude_profile"].shape[0] if (e0["tag"] + "_altitude_profile") in arr else 0
    b = flatten.HostBatch(n, k)
    if k:
        b.alt_grid[:] = arr[e0["tag"] + "_altitude_profile"]
    for i, e in enumerate(entries):
        inp = e["inputs"]
        b.ic[0:3, i] = inp["position"]
        b.ic[3:6, i] = inp["velocity"]
        b.ic[6:10, i] = inp["quaternion"]
        b.ic[10:13, i] = inp["angular_velocity"]
        b.rocket[:, i] = [inp["dry_mass"], inp["propellant_mass"]]
        if inp["motor_kind"] == 1:
            base = models.SolidMotor().thrust_curve_thrust
            cur = arr[e["tag"] + "_thrust_curve_thrust"]
            j = int(np.argmax(base))
            mult = cur[j] / base[j]
            # the multiplier must reproduce the golden's scaled curve bit for bit
            if not np.array_equal(base * mult, cur):
                cands = [cur[m] / base[m] for m in range(len(base)) if base[m] != 0]
                mult = next(c for c in cands if np.array_equal(base * c, cur))
            thrust = mult
        else:
            thrust = inp["thrust_vacuum"]
        b.motor[:, i] = [thrust, inp["nozzle_exit_area"], inp["mass_flow_rate"], inp["burn_time"]]
        if k:
            b.wind[:, :, i] = arr[e["tag"] + "_wind_profile"]
    return b


def group_flights(idx):
    """Group golden entries by (motor_kind, wind-key) so each group forms one batch."""
    groups = {}
    for e in idx:
        key = e["key"]
        kind = e["inputs"]["motor_kind"]
        if isinstance(key, list) and len(key) == 4:
            g = (kind, key[1], key[2])
        elif isinstance(key, list):
            g = (kind, "planar")
        else:
            g = (kind, key)
        groups.setdefault(g, []).append(e)
    return groups


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def synthetic_summary(n, seed):
    """A [16, n] float64 summary and an int32 status without any flight behind them, for the tests of the analysis
    workspace: apogee uniform in 50..90000, range in 0..250000, flight time in 0..700 (about 60 % of the samples pass the
    reference's outlier filter), impact x / y normal x 1000, three NaN and one inf at fixed places, end codes 0..4."""
    rng = np.random.default_rng(seed)
    summ = rng.normal(size=(_abi.SUMMARY_DIM, n))
    summ[_abi.SUM_APOGEE_ALT] = rng.uniform(50.0, 90000.0, n)
    summ[_abi.SUM_RANGE] = rng.uniform(0.0, 250000.0, n)
    summ[_abi.SUM_FLIGHT_TIME] = rng.uniform(0.0, 700.0, n)
    summ[_abi.SUM_IMPACT_X] = rng.normal(size=n) * 1000.0
    summ[_abi.SUM_IMPACT_Y] = rng.normal(size=n) * 1000.0
    summ[_abi.SUM_APOGEE_ALT, 5] = np.nan
    summ[_abi.SUM_RANGE, n // 2] = np.nan
    summ[_abi.SUM_IMPACT_X, n - 1] = np.nan
    summ[_abi.SUM_FLIGHT_TIME, 7] = np.inf
    status = rng.integers(0, 5, n).astype(np.int32)
    return summ, status


def same_nested(a, b):
    """Equality of nested dicts / lists / tuples of numbers in which a NaN equals a NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_nested(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_nested(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b):
        return True
    return type(a) is type(b) and a == b


def ulp(ref, dtype):
    """Spacing of the floating-point format `dtype` at |ref|: 2^(e - p + 1) for 2^e <= |ref| < 2^(e+1), with the
    format's denormal spacing below its smallest normal number (and at 0)."""
    fi = np.finfo(dtype)
    a = np.abs(np.asarray(ref, dtype=np.float64))
    _, e = np.frexp(a)                      # a = m 2^e with 1/2 <= m < 1
    e = np.where(a > 0, np.maximum(e - 1, fi.minexp), fi.minexp)
    return np.ldexp(1.0, e - fi.nmant)


def ulp_error(got, ref_hi, ref_lo, dtype):
    """|got - (ref_hi + ref_lo)| in ulps of `dtype` at the reference value (ref_hi + ref_lo: a high-precision
    reference split into its float64 head and tail).  A NaN or infinite `got` at a finite reference counts as inf."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs((got - ref_hi) - ref_lo) / ulp(ref_hi, dtype)
    return np.where(np.isnan(err), np.inf, err)
