"""The buffer layout of erpl_mc_compare (csrc/erpl_stat_layout.h: erpl_compare_layout) over a fixed table of sizes.  No GPU:
csrc/erpl_stat_layout_table (host compiler only) prints the offsets.  What a piece has to hold is written down HERE, from
the comments on ErplCmpArgs, ErplCorrArgs and ErplBootPrep in csrc/erpl_tables.h, not asked of the code under test; a wrong
term in the layout is an out-of-bounds write on the device.

The population buffer, sized by (n_a, n_b):
  pop_a / pop_b   the population bytes of a run: n bytes (ErplCorrArgs::pop is [n])
  src_a / src_b   the sample of every dense member of a run: at most n of them, 32 bits each (ErplBootPrep::src)
  count           the selects' own counts, one 64-bit word per run
  sel_temp        the scratch of the select: what rocPRIM asked for, never empty, whole lines of 256 bytes
The pooled buffer, sized by N = m_a + m_b (empty for N = 0), with Q = P + 1 replicates (the identity first) in
words = ceil(Q / 64) words of 64 labels, wb of them in one block of permutations:
  val[j]          the pooled values of row j: N doubles
  xy              N (x, y) pairs, with the bivariate test only
  keys, idx       the sort's keys and indices, in and out: 2 N of 64 bits, 2 N of 32 bits
  temp            the scratch of the sort
  sidx[j], r2e[j] per row the member at every sorted position (32 bits) and its doubled mid-rank with the class-end bit (64 bits)
  thr             per replicate the (key, index) pair of the threshold: words 64 pairs of 64-bit words
  bits            the label words of one block: N wb of 64 bits - at most 256 MiB unless one word per member is more than that
  cnt             per chunk of the sorted order and replicate of the block a 32-bit count: chunks wb 64
  part            per chunk and replicate of the block a record of 64 bytes; chunks wb <= 16384: at most 64 MiB
  rank            per row and replicate a record of 64 bytes: R words 64
  at_value        R doubles
  epart           per (tile of 256 members, slice, word of the block, label, sum) a double: tiles slices wb 64 3, bivariate only
  eout            words 64 3 doubles"""
import itertools
import os
import subprocess

import pytest

from test_stat_layout import TEMPS, align256, check_pieces

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "erpl_monte_carlo_sim_amd", "csrc")

BITS_MAX = 256 << 20
PAIRS = ((1, 1, 2), (255, 2, 257), (1025, 300, 1025), (40000, 30000, 54074), (65536, 65536, 65536), (1048576, 1048576, 262144),
         (1048576, 1048576, 2097152), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 32 - 2), (1000, 1000, 0))
CMP = [("cmp", na, nb, N, R, P, biv, t, t2)
       for (na, nb, N), R, P, biv, (t, t2) in itertools.product(PAIRS, (1, 4), (0, 63, 64, 999, 4096), (0, 1),
                                                                  zip(TEMPS, reversed(TEMPS)))]


def words_of(P):
    return (P + 1 + 63) // 64


def block_words(N, P):
    return max(1, min(words_of(P), (BITS_MAX // 8) // N))


def chunks_of(N, wb):
    want = min(-(-N // 256), 1024, 16384 // wb)
    length = -(-N // want)
    return -(-N // length)


def slices_of(N, wb):
    tiles = -(-N // 256)
    most = min(tiles, -(-1024 // (tiles * wb)))
    per = -(-tiles // most)
    return -(-tiles // per)


@pytest.fixture(scope="module")
def answers():
    subprocess.run(["make", "-s", "-C", CSRC, "erpl_stat_layout_table"], check=True)     # (nothing to do after build())
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in CMP)
    r = subprocess.run([os.path.join(CSRC, "erpl_stat_layout_table")], input=text, capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")
    assert len(lines) == len(CMP) + 1 and lines[-1] == ""
    return {req: [int(v) for v in line.split()] for req, line in zip(CMP, lines)}


def test_the_table_covers_the_cases_that_matter():
    assert len(CMP) == 9 * 2 * 5 * 2 * 4
    assert block_words(54074, 999) == 16 and block_words(262144, 4096) == 65            # everything at once
    assert block_words(2097152, 999) == 16 and block_words(2097152, 4096) == 16         # blocks of 1024 permutations
    assert block_words(2 ** 32 - 2, 999) == 1                                           # one word is already too much
    assert chunks_of(54074, 16) == 212 and chunks_of(262144, 65) == 252 and slices_of(257, 1) == 2


def test_compare_layout(answers):
    for req in CMP:
        _, na, nb, N, R, P, biv, temp, temp2 = req
        v = answers[req]
        assert len(v) == 8 + 3 * R + 18, req
        pop_a, src_a, pop_b, src_b, count, sel_temp, sel_bytes, pop_need = v[:8]
        assert sel_bytes >= temp, req
        first = [("pop_a", pop_a, na), ("src_a", src_a, 4 * na), ("pop_b", pop_b, nb), ("src_b", src_b, 4 * nb),
                 ("count", count, 16), ("sel_temp", sel_temp, sel_bytes)]
        check_pieces(req, first, sel_bytes, pop_need)
        assert pop_a == 0, req
        val = v[8:8 + R]
        xy, keys, idx, tmp = v[8 + R:12 + R]
        sidx, r2e = v[12 + R:12 + 2 * R], v[12 + 2 * R:12 + 3 * R]
        thr, bits, cnt, part, rank, at_value, epart, eout, temp_bytes, words, wb, chunks, slices, need = v[12 + 3 * R:]
        assert words == words_of(P), req
        if N == 0:
            assert need == 0 and wb == 0, req
            continue
        assert temp_bytes >= temp2, req
        assert (wb, chunks, slices) == (block_words(N, P), chunks_of(N, block_words(N, P)), slices_of(N, block_words(N, P))), req
        assert 1 <= wb <= words and (8 * N * wb <= BITS_MAX or wb == 1), req
        assert chunks * wb <= 16384 and 64 * chunks * wb * 64 <= 64 << 20, req
        tiles = -(-N // 256)
        pieces = ([(f"val[{j}]", val[j], 8 * N) for j in range(R)] + [("xy", xy, 16 * N if biv else 0), ("keys", keys, 16 * N),
                  ("idx", idx, 8 * N), ("temp", tmp, temp_bytes)] + [(f"sidx[{j}]", sidx[j], 4 * N) for j in range(R)] +
                  [(f"r2e[{j}]", r2e[j], 8 * N) for j in range(R)] +
                  [("thr", thr, 16 * words * 64), ("bits", bits, 8 * N * wb), ("cnt", cnt, 4 * chunks * wb * 64),
                   ("part", part, 64 * chunks * wb * 64), ("rank", rank, 64 * R * words * 64), ("at_value", at_value, 8 * R),
                   ("epart", epart, 8 * 3 * 64 * wb * tiles * slices if biv else 0), ("eout", eout, 8 * 3 * words * 64)])
        check_pieces(req, pieces, temp_bytes, need)
        assert val[0] == 0 and need <= sum(size for _, _, size in pieces) + 256 * len(pieces), req


def test_the_existing_requests_answer_as_before():
    """The new request leaves the lines of the older ones alone (the strings of tests/test_sobol_layout.py, and the ladders of
    a sobol and a dep request worked out here)."""
    text = ("corr 257 48 1 0 4113\nboot 257 4 40 65536 0 4113\ndens 257 16 1 0 4113\nsobol 1025 3 2 1000 0 4113\n"
            "dep 257 2 1 4 4 10 4113\n")
    r = subprocess.run([os.path.join(CSRC, "erpl_stat_layout_table")], input=text, capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")
    assert lines[:3] == ["0 4352 103168 105472 109824 4352 110081",
                         "0 512 1792 2048 4352 6656 8960 11264 13568 15872 18176 20480 21760 23040 24320 25600 29952 32256 36608 "
                         "102144 4352 21073664",
                         "0 512 1792 2048 6400 10752 11008 11264 13568 4352 8404232"]
    n, t = 1025, align256(4113)
    src0 = align256(2 * n)
    src1 = src0 + align256(4 * n)
    cnt = src1 + align256(4 * n)
    rec0 = cnt + 256
    rec1 = rec0 + align256(8 * n * 5)
    tmp = rec1 + align256(8 * n * 5)
    rep = tmp + t
    assert [int(x) for x in lines[3].split()] == [0, src0, src1, cnt, rec0, rec1, tmp, rep, t, rep + 8 * 1000 * 2 * 8]
    n = 257
    xs, ys = (n + 15) // 16 * 16, (2 * n + 32 + 15) // 16 * 16
    src = align256(n)
    count = src + align256(4 * n)
    yd = count + 256
    xc = yd + align256(8 * n)
    yext = xc + align256(2 * xs)
    keys = yext + align256(ys)
    idx = keys + align256(16 * n)
    temp = idx + align256(8 * n)
    cstat = temp + t
    tab = cstat + align256(8 * 6 * 2 * 4)
    null = tab + align256(8 * 2 * 4 * 4)
    assert [int(x) for x in lines[4].split()] == [0, src, count, yd, xc, yext, keys, idx, temp, cstat, tab, null, xs, ys, t,
                                                  null + 8 * 4 * 2 * 10]
