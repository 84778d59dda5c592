"""The scheduling policy of csrc/erpl_plan.h against the table of tests/golden/plan_cases.json: how the commit before the
policy became one function scheduled a batch, row by row.  No GPU: csrc/erpl_plan_table (host compiler only) prints the plans."""
import json
import os
import subprocess

import pytest

from erpl_monte_carlo_sim_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "erpl_monte_carlo_sim_amd", "csrc")
INPUTS = ("queues", "depth", "in_flight", "precision", "n", "n_traj", "adopt", "sweep_pool", "chunk", "waves", "seen_mean_steps",
          "two_priorities", "pool_on", "lane_stream", "n_cu", "max_time", "dt_flight")
COLUMNS = ("rotate", "waves_per_simd", "chunk_steps", "n_phases", "adopt_lanes", "sweep_waves", "tail", "w6", "w7", "pool_on")
STREAMS = ("none", "own", "pool")      # lane_stream going in; "main" / "own" / "pool" is the tail coming out

with open(os.path.join(HERE, "golden", "plan_cases.json")) as f:
    TABLE = json.load(f)


@pytest.fixture(scope="module")
def answers():
    """One run of the table program over the whole file: {queues: depth}, {case id: its columns}."""
    subprocess.run(["make", "-s", "-C", CSRC, "erpl_plan_table"], check=True)     # (nothing to do after build())
    lines = ["depth %d" % q for q, _ in TABLE["default_depth"]]
    for case in TABLE["cases"]:
        inp = dict(TABLE["defaults"], **case["in"])
        assert set(inp) == set(INPUTS) | {"entry"}, case["id"]
        inp["precision"] = _abi.PRECISIONS[inp["precision"]]
        inp["lane_stream"] = STREAMS.index(inp["lane_stream"])
        lines.append("plan %d " % (inp["entry"] == "submit") + " ".join(repr(inp[k]) for k in INPUTS))
    r = subprocess.run([os.path.join(CSRC, "erpl_plan_table")], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       check=True)
    out = r.stdout.split("\n")
    k = len(TABLE["default_depth"])
    assert len(out) == len(lines) + 1 and out[-1] == ""
    depths = {q: int(v) for (q, _), v in zip(TABLE["default_depth"], out[:k])}
    plans = {}
    for case, line in zip(TABLE["cases"], out[k:]):
        got = dict(zip(COLUMNS, (int(v) for v in line.split())))
        got["tail"] = ("main", "own", "pool")[got["tail"]]
        plans[case["id"]] = got
    return depths, plans


def test_the_table_is_the_one_of_the_issue():
    ids = [c["id"] for c in TABLE["cases"]]
    assert len(ids) == 39 and len(set(ids)) == 39
    assert all(set(c["out"]) == set(COLUMNS) for c in TABLE["cases"])


def test_default_depth_by_queue_count(answers):
    depths, _ = answers
    assert depths == {q: d for q, d in TABLE["default_depth"]}


@pytest.mark.parametrize("case", TABLE["cases"], ids=lambda c: c["id"])
def test_plan_of_every_row(answers, case):
    _, plans = answers
    assert plans[case["id"]] == case["out"], case["note"]
