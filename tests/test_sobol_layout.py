"""The buffer layout of erpl_mc_sobol (csrc/erpl_stat_layout.h: erpl_sobol_layout) over a fixed table of sizes.  No GPU:
csrc/erpl_stat_layout_table (host compiler only) prints the offsets.  What a piece has to hold is written down HERE, from
the comments on ErplSobolArgs, ErplCorrArgs and ErplBootPrep in csrc/erpl_tables.h and on the input layout in
include/erpl_mc.h, not asked of the code under test; a wrong term in the layout is an out-of-bounds write on the device.

  pop     the population bytes of every requested row: R rows of n bytes, row r at pop + r n (ErplCorrArgs::pop is [n])
  src[r]  the design row of every dense member of row r: at most n of them, 32 bits each (ErplBootPrep::src)
  count   the select's own count, one 64-bit word per row
  rec[r]  the records of row r: at most n members of k + 2 doubles (ErplSobolArgs::rec)
  temp    the scratch of the select: what rocPRIM asked for, never empty, whole lines of 256 bytes
  rep     [R (2 + 2 k)][B] doubles, unless the caller keeps the replicates"""
import itertools
import os
import subprocess

import pytest

from test_stat_layout import TEMPS, check_pieces

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "erpl_monte_carlo_sim_amd", "csrc")

LARGEST = (2 ** 31 - 1) // 34            # the largest n with 34 n < 2^31
SIZES = (1, 255, 256, 257, 1025, LARGEST)
SOBOL = [("sobol", n, k, R, B, keeps, t)
         for n, k, R, B, keeps, t in itertools.product(SIZES, (1, 32), (1, 4), (0, 1, 65536), (0, 1), TEMPS)]


@pytest.fixture(scope="module")
def answers():
    subprocess.run(["make", "-s", "-C", CSRC, "erpl_stat_layout_table"], check=True)     # (nothing to do after build())
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in SOBOL)
    r = subprocess.run([os.path.join(CSRC, "erpl_stat_layout_table")], input=text, capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")
    assert len(lines) == len(SOBOL) + 1 and lines[-1] == ""
    return {req: [int(v) for v in line.split()] for req, line in zip(SOBOL, lines)}


def test_the_table_is_the_one_of_the_issue():
    assert 34 * LARGEST < 2 ** 31 <= 34 * (LARGEST + 1)
    assert len(SOBOL) == 6 * 2 * 2 * 3 * 2 * 4 and TEMPS == (0, 1, 256, 4096 + 17)


def test_sobol_layout(answers):
    for req in SOBOL:
        _, n, k, R, B, keeps, temp = req
        v = answers[req]
        assert len(v) == 2 * R + 6, req
        pop, src, count, rec = v[0], v[1:1 + R], v[1 + R], v[2 + R:2 + 2 * R]
        tmp, rep, temp_bytes, need = v[2 + 2 * R:]
        assert temp_bytes >= temp, req
        pieces = ([("pop", pop, R * n)] + [(f"src[{j}]", src[j], n * 4) for j in range(R)] + [("count", count, R * 8)] +
                  [(f"rec[{j}]", rec[j], n * (k + 2) * 8) for j in range(R)] +
                  [("temp", tmp, temp_bytes), ("rep", rep, 0 if keeps else R * (2 + 2 * k) * B * 8)])
        check_pieces(req, pieces, temp_bytes, need)
        assert pop == 0 and need <= sum(size for _, _, size in pieces) + 256 * len(pieces), req


def test_the_existing_requests_answer_as_before():
    """The new request leaves the lines of the other three alone."""
    text = "corr 257 48 1 0 4113\nboot 257 4 40 65536 0 4113\ndens 257 16 1 0 4113\n"
    r = subprocess.run([os.path.join(CSRC, "erpl_stat_layout_table")], input=text, capture_output=True, text=True, check=True)
    assert r.stdout == ("0 4352 103168 105472 109824 4352 110081\n"
                        "0 512 1792 2048 4352 6656 8960 11264 13568 15872 18176 20480 21760 23040 24320 25600 29952 32256 36608 "
                        "102144 4352 21073664\n"
                        "0 512 1792 2048 6400 10752 11008 11264 13568 4352 8404232\n")
