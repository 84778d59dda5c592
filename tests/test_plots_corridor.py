"""plots.corridor_figure on bands made with NumPy (no GPU, no library): the panels, their labels, the data of the median
line and of the sample count, and the file."""
import os

import numpy as np
import pytest

pytest.importorskip("matplotlib")

from erpl_monte_carlo_sim_amd import plots  # noqa: E402

Q = [0.05, 0.25, 0.5, 0.75, 0.95]


def make_result(channels=("z", "downrange", "speed"), nodes=40, q=Q, seed=3):
    rng = np.random.default_rng(seed)
    t = 0.5 * np.arange(nodes)
    out = {"time": t, "q": list(q), "channels": list(channels), "n_counted": 1000}
    for j, name in enumerate(channels):
        cloud = (j + 1) * 100.0 * np.sin(t / 7.0)[None, :] + rng.normal(size=(1000, nodes)) * (1.0 + t)[None, :]
        cloud[:, nodes - 3:] = np.nan          # nobody is left at the last nodes
        with np.errstate(all="ignore"):
            quant = np.nanquantile(cloud, q, axis=0) if len(q) else np.zeros((0, nodes))
            out[name] = {"count": np.sum(np.isfinite(cloud), axis=0), "mean": np.nanmean(cloud, axis=0),
                         "std": np.nanstd(cloud, axis=0), "min": np.nanmin(cloud, axis=0), "max": np.nanmax(cloud, axis=0),
                         "quantiles": quant}
    return out


def panels_of(fig, n):
    """(main axes, twin axes) of the n panels: the twins share a position with their panel and are created after it."""
    axes = fig.get_axes()
    assert len(axes) == 2 * n
    main = [a for a in axes if a.get_ylabel() != "Samples"]
    twin = [a for a in axes if a.get_ylabel() == "Samples"]
    assert len(main) == n and len(twin) == n
    return main, twin


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_corridor_figure_panels_labels_and_median():
    res = make_result()
    fig = plots.corridor_figure(res)
    main, twin = panels_of(fig, 3)
    assert [a.get_ylabel() for a in main] == ["Altitude (m)", "Downrange (m)", "Speed (m/s)"]
    assert main[-1].get_xlabel() == "Time (s)" and main[0].get_xlabel() == ""
    assert "1000 samples" in main[0].get_title()
    for ax, tw, name in zip(main, twin, res["channels"]):
        (line,) = ax.get_lines()
        np.testing.assert_array_equal(line.get_xdata(), res["time"])
        np.testing.assert_array_equal(line.get_ydata(), res[name]["quantiles"][2])   # the 50 % row, NaN where it is NaN
        assert len(ax.collections) == 2                                              # 5 - 95 % and 25 - 75 %
        (count,) = tw.get_lines()
        np.testing.assert_array_equal(count.get_ydata(), res[name]["count"])
    labels = [t.get_text() for t in main[0].get_legend().get_texts()]
    assert labels == ["5 - 95 %", "25 - 75 %", "50 %"]


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_corridor_figure_with_few_or_no_quantiles():
    # two quantiles, unordered: one band, the line is the quantile nearest the median
    res = make_result(channels=("vz",), q=[0.9, 0.4])
    main, _ = panels_of(plots.corridor_figure(res), 1)
    assert main[0].get_ylabel() == "vz (m/s)" and len(main[0].collections) == 1
    np.testing.assert_array_equal(main[0].get_lines()[0].get_ydata(), res["vz"]["quantiles"][1])
    # none: the mean
    res = make_result(channels=("x", "y"), q=[])
    main, _ = panels_of(plots.corridor_figure(res), 2)
    assert len(main[0].collections) == 0
    np.testing.assert_array_equal(main[1].get_lines()[0].get_ydata(), res["y"]["mean"])


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_plot_trajectory_corridor_writes_the_file(tmp_path, capsys):
    class Analyzer:
        def _create_output_directory(self):
            return str(tmp_path)

    res = make_result(nodes=12)
    assert plots.plot_trajectory_corridor(Analyzer(), res, save_plots=False) is None
    assert not os.listdir(tmp_path)
    assert plots.plot_trajectory_corridor(Analyzer(), res) == str(tmp_path)
    path = os.path.join(str(tmp_path), "monte_carlo_corridor.png")
    assert os.path.getsize(path) > 1000
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    assert path in capsys.readouterr().out
