"""erpl_mc_corridor_bands_weighted_host (csrc/erpl_bands_w.h through ctypes) against the NumPy restatement corridor_w_ref on
every case of corridor_w_cases: the exact fields - counts, sum_w, exceed_w, every quantile, min and max, the call record - to
the bit, the doubles within erpl_mc_reweight's bar (1e-12 relative, the mean to 1e-12 * sum W |x| / S).  No GPU."""
import math

import numpy as np
import pytest

import corridor_w_cases as CW
import corridor_w_ref as R
from erpl_monte_carlo_sim_amd import analysis


def on_host(case):
    return analysis.bands_weighted_host(case["values"], case["weights"], mask=case["mask"], quantiles=case["quantiles"],
                                        thresholds=case["thresholds"], m=case["m"])


def reference(case):
    return R.bands_weighted(case["values"], case["weights"], mask=case["mask"], quantiles=case["quantiles"],
                            thresholds=case["thresholds"], m=case["m"])


@pytest.mark.parametrize("name", list(CW.CASES))
def test_host_twin_matches_the_restatement(name):
    case = CW.CASES[name]
    got, want = on_host(case), reference(case)
    CW.compare(got, want, case, name)
    assert CW.same_bytes(on_host(case), got)


def test_the_cases_hold_what_they_are_meant_to_hold():
    """Every situation the kernel can meet appears in a case - checked on the restatement, so that a case that lost its point
    fails here and not silently."""
    ref = {name: reference(case) for name, case in CW.CASES.items()}
    assert sorted(case["m"] for case in CW.CASES.values() if case["m"] not in (63, 257)) == [1, 255, 1025, 4099]
    for case in CW.CASES.values():
        C, T, ld = case["values"].shape
        assert C * T <= 10 and C <= 2 and T <= 5 and ld > case["m"] and not np.all(np.isfinite(case["values"][:, :, case["m"]:]))
    # an empty population beside a full one; a row of one repeated value
    assert ref["m1"]["count"].tolist() == [[1, 0]] and ref["m1"]["n_non_finite"].tolist() == [[0, 1]]
    m63 = ref["m63"]
    assert m63["min"][0, 1] == m63["max"][0, 1] == 2.0 and m63["var"][0, 1] == 0.0 and m63["count"][0, 1] > 40
    # zeros of both signs, NaN and both infinities among the values; W = 0 columns; a mask
    row = CW.CASES["m63"]["values"][1, 0, :63]
    assert np.signbit(row[row == 0.0]).any() and not np.signbit(row[row == 0.0]).all()
    assert np.isnan(row).any() and np.isposinf(row).any() and np.isneginf(row).any() and m63["n_non_finite"][1, 0] >= 1
    assert m63["n_zero"].min() > 0 and m63["n_masked"] > 0
    # q in {0, 1} return the extremes; 0.25 * sum_w is an integer on an all-finite row
    assert np.array_equal(CW.bits(m63["quantiles"][:, 0]), CW.bits(m63["min"])) and np.array_equal(CW.bits(m63["quantiles"][:, 3]), CW.bits(m63["max"]))
    assert m63["sum_w"][0, 1] % 4 == 0 and m63["q"][1] == 0.25
    # thresholds equal to a value of the row: the comparison is strict
    assert m63["exceed_w"][0, 0, 1] == 0 and m63["thresholds"][0][0] == 2.0
    # one column holds all but a few units of the weight - and is no member of one row
    m255 = ref["m255"]
    assert m255["max_w"] == 1000000 and m255["sum_w"][0, 0] == 1000005 and m255["sum_w"][0, 2] == 5 and m255["ess"][0, 0] < 1.0001
    # every W = 2^Q at m = 4099: sum_w above 2^53, an integer product at q = 0.25
    m4099 = ref["m4099"]
    assert m4099["Q"] == 49 and m4099["K"] == 50 and int(m4099["sum_w"][0, 0]) == 4099 << 49 > 1 << 53
    assert math.isclose(m4099["ess"][0, 0], 4099.0, rel_tol=1e-12)
    # all weights zero, and a mask that removes every column: every row empty, integers 0, doubles NaN
    for name in ("all_zero", "all_masked"):
        r = ref[name]
        assert not r["count"].any() and not r["sum_w"].any() and np.isnan(r["mean"]).all() and np.isnan(r["quantiles"]).all()
    assert ref["all_zero"]["K"] == 0 and ref["all_zero"]["n_zero"].sum() == 62 + 63
    assert ref["all_masked"]["n_counted"] == 0 and ref["all_masked"]["max_w"] > 0 and not ref["all_masked"]["n_zero"].any()


def test_constant_weights_give_the_inverted_cdf_order_statistic():
    """np.quantile(method='inverted_cdf') of the row - and not the linear rule of the unweighted bands."""
    case = CW.CASES["m4099"]
    got = on_host(case)
    x = case["values"][0, 0, :case["m"]]
    want = np.quantile(x, case["quantiles"], method="inverted_cdf")
    assert np.array_equal(CW.bits(got["quantiles"][0, :, 0]), CW.bits(want))
    assert not np.array_equal(got["quantiles"][0, :, 0], np.quantile(x, case["quantiles"]))


def test_a_weight_outside_the_admitted_range_is_refused_with_its_column():
    case = CW.CASES["m257"]
    w = case["weights"].copy()
    mask = case["mask"].copy()
    w[200] = (1 << R.q_bits(257)) + 1
    w[230] = -1
    mask[200] = 1
    with pytest.raises(Exception, match=r"weights\[200\]"):
        analysis.bands_weighted_host(case["values"], w, mask=mask, m=257)
    w[200] = 1 << R.q_bits(257)
    w[230] = 0
    assert analysis.bands_weighted_host(case["values"], w, mask=mask, m=257)["max_w"] == 1 << 52
