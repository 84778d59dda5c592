"""plots.impact_point_figure on a synthetic trace dict (no GPU, no library): the two panels, the median lines, the bands,
the keep-in outline, the exit marks and the file."""
import os

import numpy as np
import pytest

pytest.importorskip("matplotlib")

from erpl_monte_carlo_sim_amd import analysis, plots  # noqa: E402

Q = [0.05, 0.25, 0.5, 0.75, 0.95]
KEEP = [(-500.0, -500.0), (3000.0, -500.0), (3000.0, 500.0), (-500.0, 500.0)]


def make_trace(nodes=32, q=Q, keep=KEEP, seed=4):
    rng = np.random.default_rng(seed)
    t = 2.5 * np.arange(nodes)
    out = {"time": t, "q": list(q), "channels": list(analysis.IIP_CHANNELS), "n_counted": 500, "keep_in": keep,
           "exit_probability": 0.25 if keep else float("nan"), "exit_interval": (0.21, 0.29) if keep else (0.0, 1.0),
           "statistics": {"exit_time": {"count": 125 if keep else 0, "mean": 30.0, "std": 2.0, "min": 25.0, "max": 40.0,
                                        "quantiles": [27.5, 29.0, 30.0, 31.0, 35.0][:len(q)]}}}
    for j, name in enumerate(analysis.IIP_CHANNELS):
        cloud = (j + 1) * 40.0 * t[None, :] + rng.normal(size=(500, nodes)) * (5.0 + t)[None, :]
        cloud[:, :2] = np.nan   # nothing lands from the first nodes
        with np.errstate(all="ignore"):
            out[name] = {"count": np.sum(np.isfinite(cloud), axis=0), "mean": np.nanmean(cloud, axis=0),
                         "std": np.nanstd(cloud, axis=0), "min": np.nanmin(cloud, axis=0), "max": np.nanmax(cloud, axis=0),
                         "quantiles": np.nanquantile(cloud, q, axis=0) if len(q) else np.zeros((0, nodes))}
    return out


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_figure_panels_lines_bands_and_outline():
    res = make_trace()
    ax_r, ax_xy = plots.impact_point_figure(res).get_axes()
    assert ax_r.get_ylabel() == "IIP Range (m)" and "Termination" in ax_r.get_xlabel()
    assert "25.00 %" in ax_r.get_title() and "[21.00, 29.00]" in ax_r.get_title()
    median, *marks = ax_r.get_lines()
    np.testing.assert_array_equal(median.get_xdata(), res["time"])
    np.testing.assert_array_equal(median.get_ydata(), res["range"]["quantiles"][2])
    assert len(ax_r.collections) == 2                                   # 5 - 95 % and 25 - 75 %
    assert sorted(float(m.get_xdata()[0]) for m in marks) == [27.5, 29.0, 30.0, 31.0, 35.0]
    assert [t.get_text() for t in ax_r.get_legend().get_texts()] == ["5 - 95 %", "25 - 75 %", "50 %"]
    track, outline = ax_xy.get_lines()
    np.testing.assert_array_equal(track.get_xdata(), res["x"]["quantiles"][2])
    np.testing.assert_array_equal(track.get_ydata(), res["y"]["quantiles"][2])
    assert list(outline.get_xdata()) == [-500.0, 3000.0, 3000.0, -500.0, -500.0]    # closed
    assert "500 samples" in ax_xy.get_title()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_figure_without_polygon_or_quantiles():
    res = make_trace(q=[], keep=None)
    ax_r, ax_xy = plots.impact_point_figure(res).get_axes()
    assert len(ax_r.collections) == 0 and len(ax_r.get_lines()) == 1 and len(ax_xy.get_lines()) == 1
    np.testing.assert_array_equal(ax_r.get_lines()[0].get_ydata(), res["range"]["mean"])
    assert "%" not in ax_r.get_title()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_plot_impact_point_trace_writes_the_file(tmp_path, capsys):
    class Analyzer:
        def _create_output_directory(self):
            return str(tmp_path)

    res = make_trace(nodes=10)
    assert plots.plot_impact_point_trace(Analyzer(), res, save_plots=False) is None
    assert not os.listdir(tmp_path)
    assert plots.plot_impact_point_trace(Analyzer(), res) == str(tmp_path)
    path = os.path.join(str(tmp_path), "monte_carlo_impact_points.png")
    assert os.path.getsize(path) > 1000
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    assert path in capsys.readouterr().out
