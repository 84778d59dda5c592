"""What test_design_abi.py (host) and test_gpu_design.py (device) share: the shapes, erpl_mc_design_host through ctypes, and
the yardsticks of a design's values against design_ref."""
import ctypes as C

import numpy as np
from scipy import special

from erpl_monte_carlo_sim_amd import _abi

# (rows, n, block, first, count, first_row)
SHAPES = ((3, 1, 0, 0, 1, 0),
          (4, 2, 0, 0, 2, 0),
          (5, 5, 0, 0, 5, 0), (5, 17, 0, 0, 17, 0),            # both walk
          (7, 64, 0, 0, 64, 0),                                 # 4^3 exactly: no walk
          (23, 65, 0, 0, 65, 0),                                # the worst walk ratio
          (23, 4097, 0, 1, 4095, 0),                            # an odd first splits a Philox pair; count no multiple of 256
          (8, 65537, 0, 65000, 537, 0),
          (2, 1000003, 0, 995907, 4096, 0),                     # large n, a window at the end
          (6, 4096, 512, 300, 1000, 0),                         # eight replicates, the window crosses replicate borders
          (5, 300, 0, 0, 300, 314))
SEED = 7
NDTRI_BAR = 8e-15     # |z - ndtri(p)| <= NDTRI_BAR max(1, |z|): 1.06e-15 measured for the formulae, room for another log


def shape_id(s):
    return "-".join(str(v) for v in s)


def spec_of(kind, rows, n, block=0, first_row=0, seed=SEED):
    spec = _abi.ErplDesignSpec()
    spec.kind, spec.rows, spec.first_row, spec.reserved = kind, rows, first_row, 0
    spec.n, spec.block, spec.seed = n, block, seed & 0xFFFFFFFFFFFFFFFF
    return spec


def host_design(lib, kind, kinds, n, block=0, first=0, count=None, first_row=0, seed=SEED, pad=0, fill=None):
    """erpl_mc_design_host into a [rows, count + pad] array (pre-filled with `fill` where given)."""
    kinds = bytes(bytearray(kinds))
    count = n - first if count is None else count
    out = np.empty((len(kinds), count + pad))
    if fill is not None:
        out[:] = fill
    spec = spec_of(kind, len(kinds), n, block, first_row, seed)
    rc = lib.erpl_mc_design_host(C.byref(spec), kinds, first, count, out.ctypes.data, count + pad)
    assert rc == 0, lib.erpl_mc_last_error()
    return out


def assert_normals(z, p_ref):
    """Normal rows against scipy.special.ndtri of the reference's p."""
    want = special.ndtri(p_ref)
    err = np.abs(z - want) / np.maximum(1.0, np.abs(z))
    assert np.all(np.isfinite(z)) and err.max() <= NDTRI_BAR, err.max()


def ranks_in_replicates(p, m):
    """The rank of every value of the rows of p ([rows, n]) within its replicate of m columns."""
    rows, n = p.shape
    blocks = p.reshape(rows, n // m, m)
    return np.argsort(np.argsort(blocks, axis=2), axis=2).reshape(rows, n)


def additive_estimator(z):
    """The mean over the columns of sum_r c_r z_r + 0.3 z_0^2 + 0.5 z_1 z_2, c = linspace(1, 2, 20), z [20, n]."""
    c = np.linspace(1.0, 2.0, 20)
    return float(np.mean(c @ z + 0.3 * z[0] ** 2 + 0.5 * z[1] * z[2]))

