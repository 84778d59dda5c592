"""The buffer layout of erpl_mc_dependence (erpl_dep_layout in csrc/erpl_stat_layout.h) over a fixed table of sizes, through
csrc/erpl_stat_layout_table (host compiler only): no GPU.  What a piece has to hold is written down HERE, from the comments
on ErplDepArgs in csrc/erpl_tables.h and from what the kernels of csrc/erpl_dependence.hip read and write, not asked of the
code under test; a wrong term in the layout is an out-of-bounds write on the device.  The requests of the other calls answer
as before."""
import itertools
import os
import subprocess

import pytest

from test_stat_layout import CSRC, TEMPS, align256, check_pieces

SIZES = (1, 2, 15, 16, 17, 255, 256, 257, 1025, 2 ** 31 - 1)
DEP = [("dep", n, F, R, M, H, P, t)
       for n, (F, R), (M, H), P, t in itertools.product(SIZES, ((1, 1), (32, 4), (3, 2)), ((2, 2), (3, 64), (64, 64)),
                                                        (0, 1, 4096), TEMPS)]
# one request of each older kind
OLD = [("corr", 1025, 48, 1, 0, 4113), ("boot", 257, 4, 40, 65536, 0, 256), ("dens", 1025, 4, 1, 0, 0),
       ("sobol", 1025, 3, 2, 1000, 0, 4113)]


def run_table(reqs):
    subprocess.run(["make", "-s", "-C", CSRC, "erpl_stat_layout_table"], check=True)     # (nothing to do after build())
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in reqs)
    r = subprocess.run([os.path.join(CSRC, "erpl_stat_layout_table")], input=text, capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")
    assert len(lines) == len(reqs) + 1 and lines[-1] == ""
    return {req: [int(v) for v in line.split()] for req, line in zip(reqs, lines)}


@pytest.fixture(scope="module")
def answers():
    return run_table(DEP + OLD)


def test_dependence_layout(answers):
    for req in DEP:
        _, n, F, R, M, H, P, temp = req
        v = answers[req]
        pop, src, count = v[:3]
        yd = v[3:3 + R]
        xc, yext, keys, idx, tmp, cstat, tab, null, x_stride, y_stride, temp_bytes, need = v[3 + R:]
        assert temp_bytes >= temp, req
        # the table kernel: 16 class bytes per load from a 16-byte aligned row; the 20 cell bytes of a step start at
        # ((d0 + s) & ~3) <= 2 n - 2 and end below 2 n + 18: erpl_dep_extend writes the bytes below 2 n + 32
        assert x_stride % 16 == 0 and x_stride >= n and y_stride % 16 == 0 and y_stride >= 2 * n + 32, req
        assert x_stride < n + 16 and y_stride < 2 * n + 32 + 16, req
        pieces = ([("pop", pop, n), ("src", src, 4 * n), ("count", count, 8)] + [(f"yd[{j}]", yd[j], 8 * n) for j in range(R)] +
                  [("xc", xc, F * x_stride), ("yext", yext, R * y_stride), ("keys", keys, 2 * n * 8), ("idx", idx, 2 * n * 4),
                   ("temp", tmp, temp_bytes), ("cstat", cstat, R * F * M * 6 * 8), ("tab", tab, R * F * M * H * 8),
                   ("null", null, R * F * 4 * P * 8)])
        check_pieces(req, pieces, temp_bytes, need)
        assert xc % 16 == 0 and yext % 16 == 0 and keys % 8 == 0 and cstat % 8 == 0, req
        # nothing but alignment between the pieces
        assert need <= sum(align256(size) for _, _, size in pieces), req


def test_the_table_is_the_one_of_the_issue():
    assert len(DEP) == 10 * 3 * 3 * 3 * 4


def test_the_existing_requests_answer_as_before(answers):
    """The lines of the older request kinds, worked out here from the documented ladders (tests/test_stat_layout.py checks
    them over its whole table)."""
    n, V, t = 1025, 48, align256(4113)
    keys, ranks = 0, align256(16 * n)
    idx = ranks + align256(8 * n * V)
    temp = idx + align256(8 * n)
    pop = temp + t
    assert answers[("corr", 1025, 48, 1, 0, 4113)] == [keys, ranks, idx, temp, pop, t, pop + n]
    v = answers[("sobol", 1025, 3, 2, 1000, 0, 4113)]
    src0 = align256(2 * n)
    src1 = src0 + align256(4 * n)
    cnt = src1 + align256(4 * n)
    rec0 = cnt + 256
    rec1 = rec0 + align256(8 * n * 5)
    tmp = rec1 + align256(8 * n * 5)
    rep = tmp + t
    assert v == [0, src0, src1, cnt, rec0, rec1, tmp, rep, t, rep + 8 * 1000 * 2 * 8]
    assert len(answers[("boot", 257, 4, 40, 65536, 0, 256)]) == 3 + 3 * 4 + 7
    assert len(answers[("dens", 1025, 4, 1, 0, 0)]) == 11
