"""The drawing layer of erpl_monte_carlo_sim_amd.plots on NumPy-made inputs (no GPU): what it draws from bin edges and
counts is what the reference's `axes.hist(values, bins=50)` calls draw from the values of tests/golden/stats.json, with
the reference's titles, axis labels and file names (monte_carlo.py:562-707)."""
import math
import os

import numpy as np
import pytest

from erpl_monte_carlo_sim_amd import analysis, plots

import helpers as H


@pytest.fixture(scope="module")
def valid_columns():
    """The filtered population of the golden run: apogee, range, flight time of the valid samples."""
    g = H.load_json("stats.json")
    inp = g["inputs"]
    keep = [i for i in range(len(inp["apogee_altitude"])) if i != inp["none_index"]]
    cols = np.array([[inp[k][i] for i in keep] for k in ("apogee_altitude", "range", "flight_time")], dtype=np.float64)
    ok = ~analysis.outlier_mask(*cols)
    assert int(ok.sum()) == g["n_samples"]
    return cols[:, ok]


def bar_heights(ax):
    from matplotlib.patches import Rectangle
    return [p.get_height() for p in ax.patches if isinstance(p, Rectangle)]


def test_distribution_panels_are_the_references(valid_columns, tmp_path):
    hists = [np.histogram(c[np.isfinite(c)], 50) for c in valid_columns]
    fig = plots.distributions_figure([(e, c) for c, e in hists], points=(valid_columns[0], valid_columns[1]))
    axes = fig.axes
    assert len(axes) == 4
    want = (("Apogee Altitude (m)", "Frequency", "Apogee Altitude Distribution"),
            ("Range (m)", "Frequency", "Range Distribution"),
            ("Flight Time (s)", "Frequency", "Flight Time Distribution"),
            ("Apogee Altitude (m)", "Range (m)", "Range vs Apogee Altitude"))
    for ax, (xl, yl, title) in zip(axes, want):
        assert (ax.get_xlabel(), ax.get_ylabel(), ax.get_title()) == (xl, yl, title)
    for ax, values, (counts, edges) in zip(axes[:3], valid_columns, hists):
        assert bar_heights(ax) == list(np.histogram(values, 50)[0])
        assert [p.get_x() for p in ax.patches] == list(edges[:-1])
        assert np.array_equal([p.get_x() + p.get_width() for p in ax.patches][-1:], edges[-1:])
    pts = axes[3].collections[0].get_offsets()
    assert np.array_equal(np.asarray(pts), valid_columns[:2].T)
    path = plots.save_figure(fig, str(tmp_path), "monte_carlo_distributions.png")
    assert path == os.path.join(str(tmp_path), "monte_carlo_distributions.png") and os.path.getsize(path) > 10000
    import sys
    assert "matplotlib.pyplot" not in sys.modules or not sys.modules["matplotlib.pyplot"].get_fignums()   # no pyplot state


def test_fourth_panel_as_density(valid_columns):
    counts, ex, ey = np.histogram2d(valid_columns[0], valid_columns[1], bins=20)
    fig = plots.distributions_figure([np.histogram(c, 50)[::-1] for c in valid_columns], density=(counts.astype(np.int64), ex, ey))
    ax = fig.axes[3]
    mesh = ax.collections[0]
    grid = np.asarray(mesh.get_array()).reshape(20, 20)          # [y, x]
    assert np.array_equal(np.ma.filled(np.ma.masked_invalid(grid), 0), counts.T)
    assert ax.get_title() == "Range vs Apogee Altitude" and not ax.patches


def trajectories(n):
    out = []
    for i in range(n):
        t = np.linspace(0.0, 10.0 + i, 30)
        pos = np.stack([t * (1 + i), -t * 0.5, 100.0 * t - 5 * t * t], axis=1)
        out.append({"trajectory": {"time": t, "altitude": pos[:, 2].copy(), "position": pos}})
    out.append({"apogee_altitude": 1.0})     # a sample that carries no trajectory is not drawn but is counted in the title
    return out


def test_trajectory_clouds(tmp_path):
    tr = trajectories(3)
    fig = plots.trajectory_cloud_figure(tr)
    ax1, ax2 = fig.axes
    assert (ax1.get_xlabel(), ax1.get_ylabel()) == ("Time (s)", "Altitude (m)")
    assert ax1.get_title() == "Trajectory Cloud - Altitude vs Time\n(4 trajectories)"
    assert (ax2.get_xlabel(), ax2.get_ylabel()) == ("East Position (m)", "North Position (m)")
    assert ax2.get_title() == "Ground Track Cloud\n(4 trajectories)"
    assert len(ax1.lines) == 3 and len(ax2.lines) == 3
    assert np.array_equal(ax1.lines[1].get_xdata(), tr[1]["trajectory"]["time"])
    assert np.array_equal(ax2.lines[2].get_ydata(), tr[2]["trajectory"]["position"][:, 1])
    assert os.path.basename(plots.save_figure(fig, str(tmp_path), "monte_carlo_trajectories.png")) == "monte_carlo_trajectories.png"
    fig3 = plots.trajectory_cloud_3d_figure(tr)
    ax = fig3.axes[0]
    assert (ax.get_xlabel(), ax.get_ylabel(), ax.get_zlabel()) == ("East Position (m)", "North Position (m)", "Altitude (m)")
    assert ax.get_title() == "3D Trajectory Cloud (4 trajectories)" and len(ax.lines) == 3
    path = plots.save_figure(fig3, str(tmp_path), "monte_carlo_trajectories_3d.png")
    assert os.path.getsize(path) > 10000


def test_landing_figure_draws_the_dicts_ellipses(tmp_path):
    from matplotlib.patches import Circle, Ellipse
    rng = np.random.RandomState(5)
    xy = rng.multivariate_normal([300.0, -120.0], [[9e4, 3e4], [3e4, 4e4]], 4000).T
    cov = np.cov(xy, bias=True)
    w = np.linalg.eigvalsh(cov)
    levels = (0.5, 0.9, 0.99)
    disp = {"count": xy.shape[1], "mean": list(xy.mean(axis=1)), "covariance": cov.tolist(),
            "var_major": w[1], "var_minor": w[0], "angle": 0.5 * math.atan2(2 * cov[0, 1], cov[0, 0] - cov[1, 1]),
            "centre": [0.0, 0.0], "cep": float(np.median(np.hypot(*xy))),
            "ellipses": [{"level": p, "k2": -2 * math.log(1 - p), "semi_major": math.sqrt(-2 * math.log(1 - p) * w[1]),
                          "semi_minor": math.sqrt(-2 * math.log(1 - p) * w[0]), "inside": 7} for p in levels]}
    counts, ex, ey = np.histogram2d(xy[0], xy[1], bins=40)
    fig = plots.landing_figure(disp, density=(counts, ex, ey))
    ax = fig.axes[0]
    ellipses = [p for p in ax.patches if isinstance(p, Ellipse) and not isinstance(p, Circle)]
    assert len(ellipses) == 3
    for e, d in zip(ellipses, disp["ellipses"]):
        assert tuple(e.get_center()) == tuple(disp["mean"])
        assert e.get_width() == 2 * d["semi_major"] and e.get_height() == 2 * d["semi_minor"]
        assert e.get_angle() == math.degrees(disp["angle"])
    circles = [p for p in ax.patches if isinstance(p, Circle)]
    assert len(circles) == 1 and circles[0].get_radius() == disp["cep"] and tuple(circles[0].get_center()) == (0.0, 0.0)
    assert (ax.get_xlabel(), ax.get_ylabel()) == ("East Position (m)", "North Position (m)")
    path = plots.save_figure(fig, str(tmp_path), "monte_carlo_landing.png")
    assert os.path.getsize(path) > 10000
    # a degenerate cloud (inside == -1) and an empty one (NaN axes) are drawn without their content / at all
    disp["ellipses"][0]["inside"] = -1
    disp["ellipses"][1]["semi_minor"] = float("nan")
    fig = plots.landing_figure(disp, points=(xy[0][:100], xy[1][:100]))
    assert len([p for p in fig.axes[0].patches if isinstance(p, Ellipse) and not isinstance(p, Circle)]) == 2


def test_analyzer_has_the_references_plot_methods():
    from erpl_monte_carlo_sim_amd.monte_carlo import MonteCarloAnalyzer
    import inspect
    for name, params in (("plot_results", ["self", "analysis", "save_plots"]),
                         ("plot_trajectory_cloud", ["self", "analysis", "save_plots", "max_trajectories"]),
                         ("plot_trajectory_cloud_3d", ["self", "analysis", "save_plots", "max_trajectories"]),
                         ("plot_landing_dispersion", ["self", "analysis", "save_plots", "target"])):
        sig = inspect.signature(getattr(MonteCarloAnalyzer, name))
        assert list(sig.parameters) == params, name
        assert sig.parameters["save_plots"].default is True
