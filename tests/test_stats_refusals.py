"""The statistics entry points refuse bad arguments with the return codes and the erpl_mc_last_error texts recorded in
tests/golden/stats_refusals.json, byte for byte.  No GPU: every case of stats_refusal_cases.py is refused before the
context is looked at.  The file was recorded by tools/record_stats_refusals.py on the commit before the argument checks of
csrc/erpl_stats_api.hip were put together from shared pieces."""
import json
import os

import pytest

import helpers as H
import stats_refusal_cases as cases

GOLDEN = os.path.join(H.GOLDEN, "stats_refusals.json")
with open(GOLDEN) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def answers():
    return cases.collect(H.load_lib())


def test_the_recording_covers_the_cases():
    assert os.path.getsize(GOLDEN) <= 64 * 1024
    ids = [c[0] for c in cases.CASES] + [c[0] for c in cases.INDEX_CASES]
    assert len(ids) == len(set(ids))
    assert set(ids) < set(RECORDED) and len(RECORDED) == len(ids) + 6          # and the six *_defaults(NULL)
    assert all(rc == -1 and msg for rc, msg in RECORDED.values())


@pytest.mark.parametrize("cid", sorted(RECORDED))
def test_same_refusal_as_recorded(answers, cid):
    assert answers[cid] == RECORDED[cid]
