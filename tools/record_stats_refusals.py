"""Record what the statistics entry points answer to bad arguments: tests/golden/stats_refusals.json, which
tests/test_stats_refusals.py holds every later build to, return code and whole erpl_mc_last_error text.

    python tools/record_stats_refusals.py [--lib PATH/liberpl_mc.so] [--out FILE]

Needs no GPU: every case of tests/stats_refusal_cases.py is refused before the context is looked at.  Run it on a build
whose texts are the contract (the commit BEFORE a change that must leave them alone), never to make a failing comparison
pass."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import stats_refusal_cases as cases  # noqa: E402
from erpl_monte_carlo_sim_amd import _abi  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", default=None, help="another build of liberpl_mc.so (default: the package's own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stats_refusals.json"))
    args = ap.parse_args()
    rec = cases.collect(_abi.load_library(args.lib))
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(rec)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
