#!/usr/bin/env python3
"""Writes erpl_monte_carlo_sim_amd/csrc/erpl_qmc_table.inc: the Joe-Kuo direction numbers of the dimensions 1 .. 1023 of
erpl_mc_qmc, one line per dimension - the primitive polynomial (leading and trailing coefficient included, so its bit
length less one is the degree s) followed by the s initial values m_1 .. m_s.  Dimension 0 is the van der Corput sequence
and needs no entry.  The numbers are read from the copy that SciPy installs (scipy/stats/_sobol_direction_numbers.npz,
arrays `poly` and `vinit`: new-joe-kuo-6.21201); csrc/erpl_qmc.h expands them to V[1024][32] by the recurrence.

    python tools/gen_qmc_table.py            # rewrites the file
    python tools/gen_qmc_table.py --check    # exit status 1 if the committed file differs
"""
import os
import sys

import numpy as np

DIMS = 1024
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "erpl_monte_carlo_sim_amd", "csrc", "erpl_qmc_table.inc")

NOTICE = """\
// erpl_qmc_table.inc - written by tools/gen_qmc_table.py, do not edit.  Direction numbers of the Sobol' sequence for the
// dimensions 1 .. 1023 (new-joe-kuo-6.21201; S. Joe and F. Y. Kuo, "Constructing Sobol sequences with better
// two-dimensional projections", SIAM J. Sci. Comput. 30, 2635-2654, 2008), per line: the primitive polynomial with its
// leading and trailing coefficient (degree s = its bit length - 1), then m_1 .. m_s.
//
// Copyright (c) 2008, Frances Y. Kuo and Stephen Joe
// All rights reserved.
//
// Redistribution and use in source and binary forms, with or without modification, are permitted provided that the
// following conditions are met:
//
//     * Redistributions of source code must retain the above copyright notice, this list of conditions and the following
//       disclaimer.
//
//     * Redistributions in binary form must reproduce the above copyright notice, this list of conditions and the
//       following disclaimer in the documentation and/or other materials provided with the distribution.
//
//     * Neither the names of the copyright holders nor the names of the University of New South Wales and the University
//       of Waikato and its contributors may be used to endorse or promote products derived from this software without
//       specific prior written permission.
//
// THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS ``AS IS'' AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT NOT
// LIMITED TO, THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR A PARTICULAR PURPOSE ARE DISCLAIMED.  IN NO EVENT
// SHALL THE COPYRIGHT HOLDERS BE LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL, EXEMPLARY, OR CONSEQUENTIAL DAMAGES
// (INCLUDING, BUT NOT LIMITED TO, PROCUREMENT OF SUBSTITUTE GOODS OR SERVICES; LOSS OF USE, DATA, OR PROFITS; OR BUSINESS
// INTERRUPTION) HOWEVER CAUSED AND ON ANY THEORY OF LIABILITY, WHETHER IN CONTRACT, STRICT LIABILITY, OR TORT (INCLUDING
// NEGLIGENCE OR OTHERWISE) ARISING IN ANY WAY OUT OF THE USE OF THIS SOFTWARE, EVEN IF ADVISED OF THE POSSIBILITY OF SUCH
// DAMAGE.
"""


def table_text():
    import scipy.stats
    data = np.load(os.path.join(os.path.dirname(scipy.stats.__file__), "_sobol_direction_numbers.npz"))
    poly, vinit = data["poly"], data["vinit"]
    lines = [NOTICE]
    for d in range(1, DIMS):
        p = int(poly[d])
        s = p.bit_length() - 1
        m = [int(v) for v in vinit[d, :s]]
        assert 1 <= s <= 13 and p < 65536 and p & 1 and all(v & 1 and 0 < v < (2 << j) for j, v in enumerate(m)), d
        assert not vinit[d, s:].any(), d
        lines.append(", ".join(str(v) for v in [p] + m) + ",\n")
    return "".join(lines)


def main():
    text = table_text()
    if "--check" in sys.argv[1:]:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("erpl_qmc_table.inc is " + ("up to date" if same else "STALE"))
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}: {DIMS - 1} dimensions, {len(text)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
