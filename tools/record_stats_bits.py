"""Record the bits the statistics calls return: tests/golden/stats_bits.json, which tests/test_gpu_stats_bits.py holds
every later build to.

    python tools/record_stats_bits.py [--host] [--lib PATH/liberpl_mc.so] [--out FILE]

Run it on a build whose results are the contract (the commit BEFORE a change that must leave them alone), never to make a
failing comparison pass.  The inputs and the calls are those of tests/stats_bits_cases.py: the public TrajectoryEngine
calls analyze, histogram, histogram2d, dispersion and correlation only.  Refuses to record inputs whose sums do not
depend on the order of summation (pick another seed there).  --host records tests/golden/stats_host_bits.json instead:
the bootstrap and impact_density calls of collect_host_size, which pin the host halves of those two entry points."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import helpers as H  # noqa: E402
import stats_bits_cases as cases  # noqa: E402
from erpl_monte_carlo_sim_amd.engine import TrajectoryEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", default=None, help="another build of liberpl_mc.so (default: the package's own)")
    ap.add_argument("--host", action="store_true", help="record stats_host_bits.json (bootstrap, impact_density)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = cases.HOST_SIZES if args.host else cases.SIZES
    if args.out is None:
        args.out = os.path.join(ROOT, "tests", "golden", "stats_host_bits.json" if args.host else "stats_bits.json")
    for n in sizes:
        if n >= 65:
            summ, fac, _, _ = cases.make_inputs(n)
            flat = [k for k, x in enumerate(cases.rows_used(n, summ, fac)) if not cases.order_sensitive(x)]
            if flat:
                sys.exit(f"n = {n}: rows {flat} sum to the same bits in every order; pick another seed")
    eng = TrajectoryEngine(torch.device("cuda", 0), lib_path=args.lib)
    eng.set_config(H.make_config("liquid"))
    rec = cases.collect_host(eng) if args.host else cases.collect(eng)
    eng.close()
    with open(args.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, sizes {list(sizes)}")


if __name__ == "__main__":
    main()
