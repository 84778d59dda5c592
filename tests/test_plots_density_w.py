"""plots.reweighted_impact_figure and plots.plot_reweighted_impact from a hand-made dict of analysis.reweighted_impact: no GPU."""
import json
import math
import os

import numpy as np

from erpl_monte_carlo_sim_amd import plots


def hand_made_result():
    gx, gy = np.linspace(-4.0, 6.0, 41), np.linspace(-3.0, 3.0, 25)
    dens = np.exp(-0.5 * ((gx[:, None] - 1.0) ** 2 / 2.0 + gy[None, :] ** 2)) / (2 * math.pi * math.sqrt(2.0))
    peak = float(dens.max())
    zones = [{"vertices": np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0], [0.0, 2.0]]), "weight": 31 << 30, "a2": 0.02,
              "probability": 0.31, "se": 0.04, "interval": (0.2316, 0.3884)},
             {"vertices": np.array([[-3.0, -2.0], [-1.0, -2.0], [-2.0, 1.0]]), "weight": 0, "a2": 0.0, "probability": 0.0,
              "se": 0.0, "interval": (0.0, 0.0)}]
    return {"count": 100, "n_zero": 3, "sum_w": 100 << 30, "max_w": 1 << 31, "ess": 61.4, "solid": True, "grid_x": gx, "grid_y": gy,
            "density": dens, "peak": peak, "levels": [0.5, 0.9, 0.99], "thresholds": [0.5 * peak, 0.1 * peak, 0.01 * peak],
            "content_w": [51 << 30, 91 << 30, 100 << 30], "ranges": ((-4.0, 6.0), (-3.0, 3.0)), "zones": zones,
            "cep": {"q": [0.5, 0.9], "quantiles": [1.2, 2.9], "mean": 1.4, "mean_se": 0.1}, "warnings": [],
            "sample_density": object()}


def test_figure_from_a_hand_made_result():
    from matplotlib.contour import ContourSet
    from matplotlib.patches import Polygon
    res = hand_made_result()
    fig = plots.reweighted_impact_figure(res)
    ax = fig.axes[0]
    sets = [c for c in ax.collections if isinstance(c, ContourSet)]
    lines = [c for c in sets if not c.filled]
    assert len(sets) == 2 and len(lines) == 1 and list(lines[0].levels) == sorted(res["thresholds"])
    outlines = [p for p in ax.patches if isinstance(p, Polygon)]
    assert len(outlines) == 2 and np.array_equal(outlines[0].get_xy()[:4], res["zones"][0]["vertices"])
    labels = [t.get_text() for t in ax.get_legend().get_texts()]
    assert any("90 %" in s for s in labels) and any("P = 0.31" in s for s in labels)
    assert "effective 61" in ax.get_title() and "target law" in ax.get_title()
    assert "inside" not in res["zones"][0]                     # the figure works on a view, the dict is the caller's
    # not solid: the zones and the launch site, no contours
    res["solid"], res["thresholds"], res["ess"] = False, [math.nan] * 3, math.nan
    res["density"] = np.full_like(res["density"], math.nan)
    ax = plots.reweighted_impact_figure(res).axes[0]
    assert not [c for c in ax.collections if isinstance(c, ContourSet)] and len(ax.patches) == 2


def test_png_and_json(tmp_path, monkeypatch):
    class Analyzer:
        def _create_output_directory(self):
            return str(tmp_path)

    monkeypatch.setattr(plots, "DPI", 60)
    res = hand_made_result()
    assert plots.plot_reweighted_impact(Analyzer(), res, save_plots=False) is None
    out_dir = plots.plot_reweighted_impact(Analyzer(), res)
    assert out_dir == str(tmp_path) and os.path.getsize(os.path.join(out_dir, "monte_carlo_reweighted_impact.png")) > 0
    saved = json.load(open(os.path.join(out_dir, "reweighted_impact.json")))
    assert "sample_density" not in saved and "sample_density" in res
    assert saved["sum_w"] == 100 << 30 and saved["zones"][0]["weight"] == 31 << 30 and saved["zones"][0]["probability"] == 0.31
    assert saved["cep"]["quantiles"] == [1.2, 2.9] and saved["thresholds"] == res["thresholds"]
