"""plots.given_data_figure on a result made with NumPy (no GPU, no library): the panels, their labels, the delta bars, the null
band, the main-effect curves of the top factors and the file."""
import os

import numpy as np
import pytest

pytest.importorskip("matplotlib")

from erpl_monte_carlo_sim_amd import analysis, plots  # noqa: E402

NAMES = ["mass", "wind_direction", "dead_draw", "thrust", "dummy"]


def make_result(rows=("apogee_altitude", "range"), names=NAMES, shifts=200, classes=8, seed=5):
    """A hand-made dict of TrajectoryEngine.dependence, finished by analysis.finish_given_data as given_data_sensitivity
    does."""
    rng = np.random.default_rng(seed)
    R, F = len(rows), len(names)

    def measure(scale):
        est = scale * rng.random((R, F)) + 0.05
        est[:, 2] = 0.045                                # a factor inside its band
        have = shifts > 0
        return {"estimate": est, "null_mean": np.full((R, F), 0.047 if have else np.nan),
                "null_hi": np.full((R, F), 0.051 if have else np.nan),
                "exceed": np.where(est > 0.051, 0, shifts // 2) if have else np.zeros((R, F), dtype=np.int64)}

    cs = np.zeros((R, F, classes, 6))
    cs[..., 0] = 500
    cs[..., 1] = rng.normal(size=(R, F, classes))
    cs[..., 2] = 0.1 + rng.random((R, F, classes))
    cs[..., 5] = np.sort(rng.normal(size=(R, F, classes)), axis=-1)
    cs[..., 3], cs[..., 4] = cs[..., 5] - 0.1, cs[..., 5] + 0.1
    cs[0, 0, 3, 0], cs[0, 0, 3, 1:] = 0, np.nan          # an empty class
    out = {"count": 500 * classes, "classes": classes, "cells": 16, "shifts": shifts, "level": 0.95, "factor_names": list(names),
           "row_names": list(rows), "class_stats": cs, "eta2": rng.random((R, F))}
    for key in analysis.DEP_MEASURES:
        out[key] = measure(0.3)
    return analysis.finish_given_data(out)


def test_finish_adds_p_values_excess_ranking_and_curves():
    res = make_result()
    d = res["delta"]
    np.testing.assert_array_equal(d["p_value"], (d["exceed"] + 1.0) / 201.0)
    np.testing.assert_array_equal(d["excess"], np.maximum(0.0, d["estimate"] - 0.047))
    assert np.all(d["excess"][:, 2] == 0.0)
    for j in range(2):
        order = [NAMES.index(n) for n in res["ranking"][j]]
        assert sorted(order) == list(range(5)) and np.all(np.diff(d["excess"][j, order]) <= 0) and order[-1] == 2
    c = res["curves"][0]["mass"]
    assert len(c["x"]) == 7 and not np.isnan(c["mean"]).any() and c["count"].sum() == 3500     # the empty class is left out
    assert len(res["curves"][1]["dummy"]["x"]) == 8
    bare = make_result(shifts=0)
    assert np.isnan(bare["delta"]["p_value"]).all() and np.isnan(bare["delta"]["excess"]).all()
    order = [NAMES.index(n) for n in bare["ranking"][0]]
    assert np.all(np.diff(bare["delta"]["estimate"][0, order]) <= 0)           # by delta itself without a null


def test_given_data_figure_panels_bars_band_and_curves():
    res = make_result()
    fig = plots.given_data_figure(res, top=3)
    axes = fig.get_axes()
    assert len(axes) == 4                                                    # per row: the bars, the curves
    assert "8 x 16 classes" in fig._suptitle.get_text() and "200 shifts" in fig._suptitle.get_text()
    for j, row in enumerate(res["row_names"]):
        bars_ax, curve_ax = axes[2 * j], axes[2 * j + 1]
        assert bars_ax.get_ylabel() == row and f"{res['count']} samples" in bars_ax.get_title()
        bars = [p for c in bars_ax.containers if hasattr(c, "patches") for p in c.patches]
        np.testing.assert_array_equal([b.get_height() for b in bars], res["delta"]["estimate"][j])
        np.testing.assert_allclose([b.get_x() + b.get_width() / 2 for b in bars], np.arange(5))
        assert len([c for c in bars_ax.containers if not hasattr(c, "patches")]) == 1          # the null band
        lines = [ln for ln in curve_ax.get_lines() if ln.get_label() in NAMES]
        assert [ln.get_label() for ln in lines] == res["ranking"][j][:3]
        for ln in lines:
            np.testing.assert_array_equal(ln.get_ydata(), res["curves"][j][ln.get_label()]["mean"])
    assert [t.get_text() for t in axes[2].get_xticklabels()] == NAMES
    assert [t.get_text() for t in axes[0].get_legend().get_texts()] == ["delta", "null mean .. 95 %"]


def test_given_data_figure_without_a_null_and_with_nan():
    res = make_result(rows=("range",), shifts=0)
    res["delta"]["estimate"][0, 1] = np.nan                                  # e.g. an empty population
    axes = plots.given_data_figure(res).get_axes()
    assert len(axes) == 2 and all(hasattr(c, "patches") for c in axes[0].containers)            # no band without shifts
    bars = [p for c in axes[0].containers for p in c.patches]
    assert bars[1].get_height() == 0.0 and bars[0].get_height() == res["delta"]["estimate"][0, 0]


def test_plot_given_data_sensitivity_writes_the_file(tmp_path, capsys):
    class Analyzer:
        def _create_output_directory(self):
            return str(tmp_path)

    res = make_result()
    assert plots.plot_given_data_sensitivity(Analyzer(), res, save_plots=False) is None
    assert not os.listdir(tmp_path)
    assert plots.plot_given_data_sensitivity(Analyzer(), res) == str(tmp_path)
    path = os.path.join(str(tmp_path), "monte_carlo_given_data.png")
    assert os.path.getsize(path) > 1000
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    assert path in capsys.readouterr().out
