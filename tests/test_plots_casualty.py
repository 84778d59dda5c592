"""plots.casualty_figure on a synthetic result dict (no GPU, no library): the three panels, the risk map with one contour per
level that the map crosses, the outline of the population raster, Ec over the time of break-up with the contributions on a
second axis, one bar per fragment class, and the file."""
import os

import numpy as np
import pytest

pytest.importorskip("matplotlib")

from erpl_monte_carlo_sim_amd import plots  # noqa: E402


def make_result(smooth=True, times=True, bins=(24, 16), nodes=6, frags=((40.0, 0.5, 2.0), (3.0, 4.0, 150.0))):
    ex, ey = np.linspace(-1200.0, 1200.0, bins[0] + 1), np.linspace(-800.0, 800.0, bins[1] + 1)
    cx, cy = 0.5 * (ex[:-1] + ex[1:]), 0.5 * (ey[:-1] + ey[1:])
    risk = 3e-5 * np.exp(-0.5 * ((cx[:, None] - 200.0) / 300.0) ** 2 - 0.5 * (cy[None, :] / 200.0) ** 2)
    pop = np.where(cx[:, None] > 0.0, 1e-3, 1e-5) * np.ones((1, bins[1]))
    node_ec = np.linspace(1e-4, 6e-4, nodes)
    p_fail = np.full(nodes, 0.01)
    frag_ec = np.array([2.0e-5, 1.5e-5])[:len(frags)]
    return {"ec": 3.5e-5, "ec_se": 2e-6, "missing_share": 0.125, "off_grid": 7, "levels": [1e-6, 1e-5, 0.5],
            "risk_smooth": risk if smooth else None, "risk_count": np.where(risk > 1e-5, risk, 0.0), "edges_x": ex, "edges_y": ey,
            "centres_x": cx, "centres_y": cy, "population": pop, "per_node": {"ec": node_ec}, "per_fragment": {"ec": frag_ec},
            "ec_contribution": p_fail * node_ec, "p_fail": p_fail, "time": 5.0 * np.arange(nodes) if times else None,
            "fragments": list(frags)}


def test_figure_panels_contours_lines_and_bars():
    res = make_result()
    fig = plots.casualty_figure(res)
    axes = fig.get_axes()
    ax_m, ax_t, ax_f = axes[0], axes[1], axes[2]
    assert "smoothed" in ax_m.get_title() and "3.5e-05" in ax_m.get_title() and "12.5 %" in ax_m.get_title() and "7" in ax_m.get_title()
    assert ax_m.get_xlabel() == "X (m)" and ax_m.get_ylabel() == "Y (m)"
    assert len(ax_m.collections) >= 3                       # the image, the population outline, the level contours
    (line,) = ax_t.get_lines()
    np.testing.assert_array_equal(line.get_xdata(), res["time"])
    np.testing.assert_array_equal(line.get_ydata(), res["per_node"]["ec"])
    assert "Break-up" in ax_t.get_xlabel()
    twin = [a for a in axes if a is not ax_t and a.get_ylabel().startswith("p_fail")]
    assert len(twin) == 1 and len(twin[0].patches) == len(res["time"])
    np.testing.assert_allclose([p.get_height() for p in twin[0].patches], res["ec_contribution"])
    assert [p.get_height() for p in ax_f.patches] == list(res["per_fragment"]["ec"])
    assert [t.get_text() for t in ax_f.get_xticklabels()] == ["40 x 0.5 m2, 2 kg", "3 x 4 m2, 150 kg"]


def test_figure_of_a_counted_map_without_times_or_contours():
    res = make_result(smooth=False, times=False)
    res["levels"] = []
    res["population"] = None
    axes = plots.casualty_figure(res).get_axes()
    assert "counted" in axes[0].get_title() and len(axes[0].collections) == 1 and axes[1].get_xlabel() == "Node"
    np.testing.assert_array_equal(axes[1].get_lines()[0].get_xdata(), np.arange(6.0))
    one = make_result(bins=(1, 1), nodes=1, frags=((1.0, 1.0, 1.0),))   # a single cell, node and class: nothing to contour
    assert len(plots.casualty_figure(one).get_axes()[0].collections) == 1


def test_plot_writes_the_file(tmp_path):
    class Analyzer:
        def _create_output_directory(self):
            return str(tmp_path)

    out = plots.plot_casualty(Analyzer(), make_result(), True)
    assert out == str(tmp_path) and os.path.getsize(os.path.join(out, "monte_carlo_casualty.png")) > 10000
    assert plots.plot_casualty(Analyzer(), make_result(), False) is None
