"""erpl_mc_corridor_drivers_defaults / erpl_mc_corridor_drivers at the C boundary, as far as it goes without a GPU: the
declarations, the structs and the constants against gcc, the defaults, every argument check in the order the header states
(they come before any device work and look at the context last, so a NULL context and dummy pointers that are never
dereferenced show them all), the host-side refusals of the engine method, the host rules through erpl_cdrv_check and the
workspace layout through erpl_stat_layout_table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from erpl_monte_carlo_sim_amd import _abi, analysis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc")
NAMES = ("erpl_mc_corridor_drivers_defaults", "erpl_mc_corridor_drivers")


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


def test_symbols_are_declared_listed_documented_and_exported(lib):
    hdr = open(os.path.join(REPO, "include", "erpl_mc.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _abi.EXPORTS and f"int {name}(" in hdr and name in doc, name
        getattr(lib, name)


def test_structs_and_constants_match_the_c_compiler(tmp_path):
    macros = (("ERPL_CDRV_MAX_FACTORS", _abi.CDRV_MAX_FACTORS), ("ERPL_CDRV_MAX_ROWS", _abi.CDRV_MAX_ROWS),
              ("ERPL_CORR_MAX_FACTORS", _abi.CDRV_MAX_FACTORS))
    H.check_struct_layouts(tmp_path, (("erpl_cdrv_spec", "ErplCdrvSpec"), ("erpl_cdrv_result", "ErplCdrvResult"),
                                      ("erpl_cdrv_row", "ErplCdrvRow")), macros)
    assert _abi.CDRV_MAX_FACTORS == 32 and _abi.CDRV_MAX_ROWS == 8 * 4096 == _abi.CORRIDOR_MAX_CHANNELS * _abi.CORRIDOR_MAX_NODES
    assert _abi.ABI_VERSION == 4
    # the engine reads an array of erpl_cdrv_row as 8 eight-byte words per record, the two flags in the last one
    assert C.sizeof(_abi.ErplCdrvRow) == 64 and _abi.ErplCdrvRow.constant.offset == 56 and _abi.ErplCdrvRow.regression_ok.offset == 60


def test_defaults(lib):
    s = _abi.ErplCdrvSpec()
    C.memset(C.byref(s), 0xff, C.sizeof(s))
    assert lib.erpl_mc_corridor_drivers_defaults(C.byref(s)) == 0
    assert (s.n_factors, s.n_rows, s.regression, s.reserved) == (0, 0, 1, 0)
    assert lib.erpl_mc_corridor_drivers_defaults(None) == -1 and "spec" in lib.erpl_mc_last_error().decode()


def test_checks_come_before_any_device_work_in_the_stated_order(lib):
    D = H.DUMMY

    def spec(n_factors=3, n_rows=7, regression=1):
        s = _abi.ErplCdrvSpec()
        s.n_factors, s.n_rows, s.regression = n_factors, n_rows, regression
        return s

    def call(s, factors=D, ldf=5, values=D, ld=5, m=5, result=True, rows=D, pearson=D, src=D):
        res = _abi.ErplCdrvResult()
        rc = lib.erpl_mc_corridor_drivers(None, factors, ldf, values, ld, None, m, C.byref(s) if s is not None else None,
                                          C.byref(res) if result else None, rows, pearson, src, None)
        return rc, lib.erpl_mc_last_error().decode()

    def refused(word, *a, **kw):
        rc, msg = call(*a, **kw)
        assert rc == -1 and word in msg, (word, msg)

    bad = spec(0, 0, 2)   # every field wrong: what is checked before the fields is still named first
    # 1. the pointers, in the order spec, factors, values, result, rows, pearson
    refused("spec", None, None, -1, None, -1, 0, False, None, None, None)
    refused("factors", bad, None, -1, None, -1, 0, False, None, None, None)
    refused("values", bad, D, -1, None, -1, 0, False, None, None, None)
    refused("result", bad, D, -1, D, -1, 0, False, None, None, None)
    refused("rows", bad, D, -1, D, -1, 0, True, None, None, None)
    refused("pearson", bad, D, -1, D, -1, 0, True, D, None, None)
    # 2. m, then ld, then ldf
    for m in (0, -3, 1 << 31, 1 << 40):
        refused(f"m = {m}", bad, D, -1, D, -1, m, True, D, D, None)
    refused("ld = 4", bad, D, 3, D, 4, 5, True, D, D, None)
    refused("ldf = 3", bad, D, 3, D, 5, 5, True, D, D, None)
    # 3. the spec: n_factors, n_rows, regression
    for f in (0, -1, 33):
        refused("n_factors", spec(f, 0, 2), src=None)
    for r in (0, -1, _abi.CDRV_MAX_ROWS + 1):
        refused("n_rows", spec(3, r, 2), src=None)
    for g in (-1, 2):
        refused("regression", spec(3, 7, g), src=None)
    # 4. src against regression
    refused("src", spec(regression=0))
    refused("src", spec(regression=1), src=None)
    # 5. only the context is left
    refused("ctx", spec())
    refused("ctx", spec(regression=0), src=None)
    refused("ctx", spec(32, _abi.CDRV_MAX_ROWS, 1), ldf=(1 << 31) - 1, ld=1 << 40, m=(1 << 31) - 1)
    refused("ctx", spec(1, 1, 1), ldf=1, ld=1, m=1)


def test_engine_method_refuses_host_tensors_and_wrong_dtypes():
    """No CPU path behind the call: the refusals are on the host, before the library is called (the engine here has no
    library and no context)."""
    import torch
    from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine
    eng = object.__new__(TrajectoryEngine)
    eng.device = torch.device("cuda", 0)
    f64, f32 = torch.zeros((3, 8), dtype=torch.float64), torch.zeros((3, 8), dtype=torch.float32)
    with pytest.raises(ValueError, match="factors"):
        TrajectoryEngine.corridor_drivers(eng, f64, torch.zeros((2, 4, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="factors"):
        TrajectoryEngine.corridor_drivers(eng, f32, f64)
    with pytest.raises(ValueError, match="factors"):
        TrajectoryEngine.corridor_drivers(eng, None, None)
    with pytest.raises(ValueError, match="factor names"):
        analysis.corridor_drivers(f64, f64, ["a", "b"], engine=eng)


def test_ranking_share_and_lead():
    names = ["a", "b", "c"]
    pearson = np.array([[[0.9, -0.1, np.nan], [0.2, -0.8, np.nan], [np.nan, np.nan, np.nan], [0.5, 0.5, np.nan]]])
    count = np.array([[10, 10, 1, 10]])
    share, ranking, lead = analysis.rank_corridor_drivers(pearson, count, names)
    assert np.allclose(share[0, 0, :2], [0.81, 0.01]) and np.isnan(share[0, 0, 2])
    assert ranking == [["a", "b", "c"]] and lead == [["a", "b", None, "a"]]


def test_host_rules_check_runs_clean(lib):
    exe = os.path.join(CSRC, "erpl_cdrv_check")
    assert os.path.exists(exe), "make all builds it"
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok erpl_cdrv_check"), out.stdout + out.stderr


FIELDS = ("base", "count", "fstat", "rstat", "mpart", "part", "sums", "pairs", "ext", "seg_len", "slice_len", "segs", "slices",
          "chunk_tiles", "row_doubles", "need")


def _layout(requests):
    exe = os.path.join(CSRC, "erpl_stat_layout_table")
    out = subprocess.run([exe], input="".join(r + "\n" for r in requests), capture_output=True, text=True, check=True)
    return [dict(zip(FIELDS, (int(v) for v in line.split()))) for line in out.stdout.splitlines()]


def test_layout_pieces_are_aligned_disjoint_and_need_is_their_end(lib):
    cases = [(m, R, F, g) for m in (1, 255, 256, 257, (1 << 31) - 1) for R in (1, 32768) for F in (1, 32) for g in (0, 1)]
    got = _layout([f"cdrv {m} {R} {F} {g}" for m, R, F, g in cases])
    assert len(got) == len(cases)
    for (m, R, F, g), l in zip(cases, got):
        P = F * (F + 1) // 2 if g else F
        rd = l["row_doubles"]
        assert rd % 4 == 0 and rd >= 2 * 48 + 16 * ((P + 15) // 16) + 1
        assert l["segs"] * l["seg_len"] >= m > (l["segs"] - 1) * l["seg_len"] and l["seg_len"] % 256 == 0 and 1 <= l["segs"] <= 64
        assert l["slices"] * l["slice_len"] >= m > (l["slices"] - 1) * l["slice_len"] and l["slice_len"] % 16 == 0
        assert 1 <= l["slices"] <= 32 and l["chunk_tiles"] >= 1
        tiles = min((R + 31) // 32, l["chunk_tiles"])
        tile = 8 * 32 * rd
        sizes = (("base", m), ("count", 32), ("fstat", 64 * F), ("rstat", 64 * R), ("mpart", 32 * max(R, F) * l["segs"]),
                 ("part", tile * tiles * l["slices"]), ("sums", tile * tiles), ("pairs", 8 * R * F), ("ext", 16 * R * F))
        end = 0
        for name, size in sizes:
            assert l[name] % 256 == 0 and l[name] >= end, (name, m, R, F, g)
            end = l[name] + size
        assert l["need"] == end
        assert tile * tiles * l["slices"] <= max(256 << 20, tile * l["slices"])
