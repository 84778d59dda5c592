"""What test_qmc_abi.py (host) and test_gpu_qmc.py (device) share: the shapes, erpl_mc_qmc_host through ctypes, the bar of the
normal rows (design_cases')."""
import ctypes as C

import numpy as np

from erpl_monte_carlo_sim_amd import _abi

import design_cases as DC

SEED = DC.SEED
# (rows, n, block, first, count, first_row, dims, pad)
SHAPES = ((5, 64, 0, 0, 64, 0, None, "random"),
          (7, 96, 32, 17, 50, 3, None, "random"),                                  # three replicates, no power of two, an odd first
          (4, 2 ** 31 - 1, 0, 2 ** 30 + 12345, 64, 0, None, "random"),             # bit 30 of the index
          (5, 300, 0, 0, 300, 0, (3, -1, 0, 1023, -1), "random"),                  # mixed: pad rows between Sobol' rows
          (5, 300, 0, 0, 300, 0, (3, -1, 0, 1023, -1), "lhs"),
          (5, 300, 100, 31, 250, 1021, None, "lhs"),                               # dims == NULL runs out of dimensions at row 1024
          (600, 300, 100, 31, 250, 500, None, "lhs"))      # more rows than one launch takes (512); the second starts on Sobol' rows
PADS = {"random": _abi.DESIGN_RANDOM, "lhs": _abi.DESIGN_LHS}


def shape_id(s):
    return "-".join("x" if v is None else "".join(str(v).split()) for v in s)


def spec_of(rows, n, block=0, first_row=0, seed=SEED, scramble=_abi.QMC_OWEN, pad=_abi.DESIGN_RANDOM):
    spec = _abi.ErplQmcSpec()
    spec.rows, spec.first_row, spec.scramble, spec.pad = rows, first_row, scramble, pad
    spec.n, spec.block, spec.seed = n, block, seed & 0xFFFFFFFFFFFFFFFF
    return spec


def dims_array(dims):
    return None if dims is None else (C.c_int32 * len(dims))(*dims)


def host_qmc(lib, kinds, n, block=0, first=0, count=None, first_row=0, dims=None, seed=SEED, scramble=_abi.QMC_OWEN,
             pad=_abi.DESIGN_RANDOM, extra=0, fill=None):
    """erpl_mc_qmc_host into a [rows, count + extra] array (pre-filled with `fill` where given)."""
    kinds = bytes(bytearray(kinds))
    count = n - first if count is None else count
    out = np.empty((len(kinds), count + extra))
    if fill is not None:
        out[:] = fill
    spec = spec_of(len(kinds), n, block, first_row, seed, scramble, pad)
    rc = lib.erpl_mc_qmc_host(C.byref(spec), kinds, dims_array(dims), first, count, out.ctypes.data, count + extra)
    assert rc == 0, lib.erpl_mc_last_error()
    return out


def interaction_estimator(z):
    """The mean over the columns of sum_{a < b} z_a z_b + sum_a z_a, z [4, n]: expectation 0, variance carried by the pairs."""
    s = z.sum(axis=0)
    return float(np.mean((s * s - (z * z).sum(axis=0)) / 2.0 + s))
