"""Record the bits the flight kernels return: tests/golden/flight_bits_*.npy, which tests/test_gpu_flight_bits.py holds
every later build to.

    python tools/record_flight_bits.py [--lib PATH/liberpl_mc.so] [--out DIR]

Run it on a build whose results are the contract (the commit BEFORE a change that must leave them alone), never to make a
failing comparison pass.  The batches and the calls are those of tests/flight_bits_cases.py.  Refuses to write anything
unless every Set S recording has a flight that ends on the ground, one that leaves through the altitude limit, one that
runs out of time and one that turned NaN, the parachute case a flight under the parachute, and the steered case a coast
time-out, an altitude exit, a landing and a flight that ran out of time."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flight_bits_cases as cases  # noqa: E402
from erpl_monte_carlo_sim_amd import _abi  # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", default=None, help="another build of liberpl_mc.so (default: the package's own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    eng = TrajectoryEngine(torch.device("cuda", 0), lib_path=args.lib)
    files, refused = {}, []
    for precision in cases.PRECISIONS:
        for case in cases.CASES:
            rec = cases.collect(eng, case, precision)
            st = cases.status_of(rec["flight"])
            ends = np.bincount(st & 0xFF, minlength=5).tolist()
            print("%-13s %-8s ends %s  nan %d  chute %d  incomplete %d" % (
                case, precision, dict(zip(_abi.END_NAMES, ends)), np.count_nonzero(st & _abi.ST_NAN),
                np.count_nonzero(st & _abi.ST_CHUTE), np.count_nonzero(st & _abi.ST_INCOMPLETE)))
            miss = cases.missing_ends(case, rec["flight"])
            if miss or np.any(st & _abi.ST_INCOMPLETE):
                refused.append("%s %s: no %s" % (case, precision, ", ".join(miss) or "complete batch"))
            for name, a in rec.items():
                files[cases.file_name(case, precision, name)] = a
    eng.close()
    if refused:
        sys.exit("nothing written:\n  " + "\n  ".join(refused))
    os.makedirs(args.out, exist_ok=True)
    for fn, a in files.items():
        np.save(os.path.join(args.out, fn), a)
    print("%d files, %d bytes in %s" % (len(files), sum(a.nbytes for a in files.values()), args.out))


if __name__ == "__main__":
    main()
