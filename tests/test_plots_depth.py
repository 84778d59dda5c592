"""plots.functional_boxplot_figure on a result made with the NumPy restatement (no GPU, no library): the panels, the median
flight's line, the outlying flights drawn one by one, and the file."""
import os

import numpy as np
import pytest

pytest.importorskip("matplotlib")

import depth_ref as R  # noqa: E402
from erpl_monte_carlo_sim_amd import analysis, plots  # noqa: E402


def make_result():
    """What analysis.trajectory_depth returns, from the restatement on the demonstration curves."""
    v = R.demo_curves()
    r = R.reference(v)
    n = v.shape[2]
    d, flags = analysis.outliergram(r["depth"][0], r["mei"][0], n)
    med = int(r["median"][0])
    ch = {"depth": r["depth"][0], "mei": r["mei"][0], "nodes": r["nodes"][0], "median": med, "median_curve": v[0, :, med],
          "central": {"lo": r["central_lo"][0], "hi": r["central_hi"][0]}, "fence": {"lo": r["fence_lo"][0], "hi": r["fence_hi"][0]},
          "whisker": {"lo": r["whisker_lo"][0], "hi": r["whisker_hi"][0]}, "count": r["count"][0], "n_defined": int(r["n_defined"][0]),
          "n_central": int(r["n_central"][0]),
          "magnitude_outliers": [{"column": int(j), "first_node": int(r["first_out"][0][j]), "nodes": int(r["n_out"][0][j])}
                                 for j in np.flatnonzero(r["n_out"][0] > 0)],
          "shape_outliers": [int(j) for j in np.flatnonzero(flags)], "outliergram_distance": d}
    return {"time": 0.5 * np.arange(v.shape[1]), "channels": ["z"], "central_share": 0.5, "factor": 1.5, "n_masked": 0,
            "warnings": [], "z": ch}, v


def test_functional_boxplot_panels_median_and_outliers(tmp_path):
    res, v = make_result()
    fig = plots.functional_boxplot_figure(res, v)
    (ax,) = fig.get_axes()
    assert ax.get_ylabel() == "Altitude (m)" and ax.get_xlabel() == "Time (s)"
    assert "400 flights" in ax.get_title() and "1 leave the fences" in ax.get_title() and "1 shape outliers" in ax.get_title()
    lines = {ln.get_label(): ln for ln in ax.get_lines()}
    med = lines[f"median flight (sample {res['z']['median']})"]
    np.testing.assert_array_equal(med.get_ydata(), v[0, :, res["z"]["median"]])
    np.testing.assert_array_equal(lines["magnitude outliers"].get_ydata(), v[0, :, 1])
    np.testing.assert_array_equal(lines["shape outliers"].get_ydata(), v[0, :, 0])
    assert len(ax.get_lines()) == 5   # two whiskers, two outliers, the median
    path = plots.save_figure(fig, str(tmp_path), "monte_carlo_functional_boxplot.png")
    assert os.path.getsize(path) > 0


def test_functional_boxplot_without_values_and_without_an_outliergram():
    res, _ = make_result()
    res["z"]["shape_outliers"] = None
    fig = plots.functional_boxplot_figure(res)
    (ax,) = fig.get_axes()
    assert len(ax.get_lines()) == 3 and "no outliergram" in ax.get_title()
