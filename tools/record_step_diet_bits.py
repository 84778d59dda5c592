"""Record the bits the fp64 throughput build returns on the mixed waves of tests/step_diet_cases.py:
tests/golden/step_diet_bits_*.npy, which tests/test_gpu_step_diet_bits.py holds every later build to.

    python tools/record_step_diet_bits.py [--lib PATH/liberpl_mc.so] [--out DIR]

Run it on a build whose results are the contract (the commit BEFORE a change that must leave them alone), never to make a
failing comparison pass.  Refuses to write anything unless every wave of every recording holds lanes on both sides of the
branches the cases are built for (step_diet_cases.missing)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import step_diet_cases as cases  # noqa: E402
from erpl_monte_carlo_sim_amd import _abi  # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", default=None, help="another build of liberpl_mc.so (default: the package's own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    eng = TrajectoryEngine(torch.device("cuda", 0), lib_path=args.lib)
    files, refused = {}, []
    for n in cases.SIZES:
        for mode in cases.MODES:
            flight = cases.collect(eng, n, mode)
            st = flight[16].astype(np.int64)
            print("%3d %-6s ends %s  nan %d  chute %d  above the hand-over speed %d" % (
                n, mode, dict(zip(_abi.END_NAMES, np.bincount(st & 0xFF, minlength=5).tolist())),
                np.count_nonzero(st & _abi.ST_NAN), np.count_nonzero(st & _abi.ST_CHUTE),
                np.count_nonzero(flight[_abi.SUM_MAX_SPEED] > 1e6)))
            refused += ["%d %s: no %s" % (n, mode, m) for m in cases.missing(flight)]
            enc = cases.encode(flight)
            if files.setdefault(cases.file_name(n), enc).tobytes() != enc.tobytes():
                refused.append("%d %s: not the bytes of %s" % (n, mode, cases.MODES[0]))
    eng.close()
    if refused:
        sys.exit("nothing written:\n  " + "\n  ".join(refused))
    os.makedirs(args.out, exist_ok=True)
    for fn, a in files.items():
        np.save(os.path.join(args.out, fn), a)
    print("%d files, %d bytes in %s" % (len(files), sum(a.nbytes for a in files.values()), args.out))


if __name__ == "__main__":
    main()
