"""erpl_mc_legacy_random_streams_device and erpl_mc_legacy_wind_profiles_device at the C boundary, as far as it goes
without a GPU: the symbols, and every argument check (they come before any device work and look at the context last, so
a NULL context and a dummy pointer that is never dereferenced show them all)."""
import ctypes as C
import os

import numpy as np
import pytest

from erpl_monte_carlo_sim_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = C.c_void_p(0x1000)
NAMES = ("erpl_mc_legacy_random_streams_device", "erpl_mc_legacy_wind_profiles_device")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _abi.load_library()


def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)
    assert lib.erpl_mc_abi_version() == 4 and _abi.ABI_VERSION == 4
    assert "#define ERPL_LEGACY_DEVICE_MAX_OUTPUTS 4096" in hdr
    assert _abi.LEGACY_DEVICE_MAX_OUTPUTS == 4096 >= 3 * _abi.MAX_WIND_KNOTS


def ops_buf(codes):
    a = np.ascontiguousarray(codes, dtype=np.uint8)
    return a, C.c_void_p(a.ctypes.data)


def test_stream_argument_checks_come_before_any_device_work(lib):
    keep, good = ops_buf([_abi.RS_GAUSS, _abi.RS_DOUBLE, _abi.RS_GAUSS])

    def call(n=8, m=3, seeds=DUMMY, ops=good, out=DUMMY):
        rc = lib.erpl_mc_legacy_random_streams_device(None, seeds, n, ops, m, out, 0, None)
        return rc, lib.erpl_mc_last_error().decode()

    rc, msg = call(n=-1)
    assert rc == -1 and "n = -1" in msg
    rc, msg = call(m=-2)
    assert rc == -1 and "m = -2" in msg
    rc, msg = call(n=2 ** 31)
    assert rc == -1 and f"n = {2 ** 31}" in msg
    rc, msg = call(m=4097, ops=DUMMY)
    assert rc == -1 and "m = 4097" in msg and "ERPL_LEGACY_DEVICE_MAX_OUTPUTS" in msg
    for name in ("seeds", "ops", "out"):
        rc, msg = call(**{name: None})
        assert rc == -1 and name in msg and "NULL" in msg
    bad_keep, bad = ops_buf([_abi.RS_GAUSS, 7, _abi.RS_GAUSS])
    rc, msg = call(ops=bad)
    assert rc == -1 and "ops[1] = 7" in msg
    # everything in order, at the limits: only the context is left
    rc, msg = call()
    assert rc == -1 and "ctx" in msg
    big_keep, big = ops_buf([_abi.RS_GAUSS] * 4096)
    rc, msg = call(n=2 ** 31 - 1, m=4096, ops=big)
    assert rc == -1 and "ctx" in msg
    # nothing to do: as on the host, before the buffers and the context are looked at
    assert call(n=0)[0] == 0 and call(m=0)[0] == 0
    assert lib.erpl_mc_legacy_random_streams_device(None, None, 0, None, 3, None, 0, None) == 0


def test_wind_argument_checks_come_before_any_device_work(lib):
    names = ("seeds", "sigma", "rho", "innov", "base", "mean_scale", "speed", "cdir", "sdir", "wind")

    def call(n=8, k=4, **kw):
        p = {name: DUMMY for name in names}
        p.update(kw)
        rc = lib.erpl_mc_legacy_wind_profiles_device(None, p["seeds"], n, k, p["sigma"], p["rho"], p["innov"], p["base"],
                                                     p["mean_scale"], p["speed"], p["cdir"], p["sdir"], p["wind"], 0, None)
        return rc, lib.erpl_mc_last_error().decode()

    rc, msg = call(n=-3)
    assert rc == -1 and "n = -3" in msg
    rc, msg = call(k=-1)
    assert rc == -1 and "k = -1" in msg
    rc, msg = call(n=2 ** 31)
    assert rc == -1 and f"n = {2 ** 31}" in msg
    rc, msg = call(k=1025)
    assert rc == -1 and "k = 1025" in msg and "ERPL_MAX_WIND_KNOTS" in msg
    for name in ("seeds", "sigma", "rho", "innov", "wind"):
        rc, msg = call(**{name: None})
        assert rc == -1 and name in msg and "NULL" in msg
    for name in ("mean_scale", "speed", "cdir", "sdir"):
        rc, msg = call(base=None, **{name: None})
        assert rc == -1 and name in msg and "NULL" in msg
        rc, msg = call(**{name: None})      # with a baseline profile the mean-wind inputs are not needed
        assert rc == -1 and "ctx" in msg
    # both modes in order, at the limits: only the context is left
    for base in (DUMMY, None):
        rc, msg = call(n=2 ** 31 - 1, k=1024, base=base)
        assert rc == -1 and "ctx" in msg
    assert call(n=0)[0] == 0 and call(k=0)[0] == 0
    assert call(n=0, seeds=None, wind=None)[0] == 0


@pytest.mark.parametrize("csv", [True, False])
def test_a_batch_without_its_wind_table_keeps_what_the_table_is_made_from(csv):
    """flatten.dispersed_batch(with_wind=False): everything but the table, plus the per-sample mean-wind inputs."""
    from erpl_monte_carlo_sim_amd import flatten, models
    import helpers as H
    P = flatten.generate_parameter_arrays(H.UNCERTAINTY, 70)
    kw = dict(base_altitude_profile=H.CSV_ALT, base_wind_profile=H.CSV_WIND) if csv else {}
    args = (models.Rocket(), models.LiquidMotor(), models.WindModel(), H.EXAMPLE_IC, P)
    full = flatten.dispersed_batch(*args, **kw)
    bare = flatten.dispersed_batch(*args, with_wind=False, **kw)
    assert bare.wind is None and full.wind.shape == (len(full.alt_grid), 3, 70)
    for name in ("ic", "rocket", "motor", "alt_grid"):
        assert np.array_equal(getattr(bare, name), getattr(full, name)), name
    assert bare.n == 70 and bare.k_wind == (6 if csv else 100)
    assert np.array_equal(bare.wind_speed, P["wind_speed"])
    assert np.array_equal(bare.wind_cos, np.cos(P["wind_direction"])) and np.array_equal(bare.wind_sin, np.sin(P["wind_direction"]))
    # the table is a function of exactly these: the host function rebuilds it from them
    seeds = P["random_seed"].astype(np.uint32)
    if csv:
        w = flatten.legacy_wind_profiles(models.WindModel(), bare.alt_grid, seeds, base=H.CSV_WIND)
        w[:, 0, :] += bare.wind_speed * bare.wind_cos
        w[:, 1, :] += bare.wind_speed * bare.wind_sin
    else:
        w = flatten.legacy_wind_profiles(models.WindModel(), bare.alt_grid, seeds, speed=bare.wind_speed, cdir=bare.wind_cos,
                                         sdir=bare.wind_sin)
    assert np.array_equal(w, full.wind)
