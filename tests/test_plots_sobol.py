"""plots.sobol_figure on indices made with NumPy (no GPU, no library): the panels, their labels, the heights of the paired
bars, the whiskers and the file."""
import os

import numpy as np
import pytest

pytest.importorskip("matplotlib")

from erpl_monte_carlo_sim_amd import plots  # noqa: E402

NAMES = ["mass", "motor_thrust", "dead_draw", "turbulence"]


def make_result(rows=("first_apogee_altitude", "rail_exit_speed"), names=NAMES, replicates=True, seed=5):
    rng = np.random.default_rng(seed)
    R, k = len(rows), len(names)

    def stat(est):
        spread = 0.02 + 0.01 * rng.random(est.shape)
        nan = np.full(est.shape, np.nan)
        return {"estimate": est, "rep_mean": est if replicates else nan, "se": spread / 2 if replicates else nan,
                "lo": est - spread if replicates else nan, "hi": est + spread if replicates else nan,
                "finite": np.full(est.shape, 1000 if replicates else 0)}

    first = rng.dirichlet(np.ones(k + 1), size=R)[:, :k]
    total = first + 0.1 * rng.random((R, k))
    first[:, 2] = total[:, 2] = 0.0                  # a factor that reaches nothing
    return {"n_base": 4096, "n_factors": k, "group_names": list(names), "row_names": list(rows), "count": np.full(R, 4000),
            "first": stat(first), "total": stat(total), "sum_first": first.sum(axis=1), "interaction": 1.0 - first.sum(axis=1)}


def test_sobol_figure_panels_bars_and_whiskers():
    res = make_result()
    fig = plots.sobol_figure(res)
    axes = fig.get_axes()
    assert len(axes) == 2
    assert [a.get_ylabel() for a in axes] == ["first_apogee_altitude", "rail_exit_speed"]
    assert [t.get_text() for t in axes[-1].get_xticklabels()] == NAMES
    assert "4096 x 6 flights" in fig._suptitle.get_text()
    for j, ax in enumerate(axes):
        bars = [p for c in ax.containers if hasattr(c, "patches") for p in c.patches]
        assert len(bars) == 2 * len(NAMES)
        np.testing.assert_array_equal([b.get_height() for b in bars[:4]], res["first"]["estimate"][j])
        np.testing.assert_array_equal([b.get_height() for b in bars[4:]], res["total"]["estimate"][j])
        # S1 left of ST, a pair per group
        np.testing.assert_allclose([b.get_x() + b.get_width() / 2 for b in bars[:4]], np.arange(4) - 0.2)
        np.testing.assert_allclose([b.get_x() + b.get_width() / 2 for b in bars[4:]], np.arange(4) + 0.2)
        assert f"interaction {res['interaction'][j]:.3f}" in ax.get_title() and "4000 design rows" in ax.get_title()
        whiskers = [c for c in ax.containers if not hasattr(c, "patches")]
        assert len(whiskers) == 2                                            # one errorbar set per index
    labels = [t.get_text() for t in axes[0].get_legend().get_texts()]
    assert labels == ["S1 (first order)", "ST (total effect)"]


def test_sobol_figure_without_replicates_and_with_nan_indices():
    res = make_result(rows=("range",), replicates=False)
    res["first"]["estimate"][0, 1] = np.nan          # e.g. a constant row
    (ax,) = plots.sobol_figure(res).get_axes()
    assert all(hasattr(c, "patches") for c in ax.containers)                 # no whiskers without intervals
    bars = [p for c in ax.containers for p in c.patches]
    assert bars[1].get_height() == 0.0 and bars[0].get_height() == res["first"]["estimate"][0, 0]


def test_plot_sobol_writes_the_file(tmp_path, capsys):
    class Analyzer:
        def _create_output_directory(self):
            return str(tmp_path)

    res = make_result()
    assert plots.plot_sobol(Analyzer(), res, save_plots=False) is None
    assert not os.listdir(tmp_path)
    assert plots.plot_sobol(Analyzer(), res) == str(tmp_path)
    path = os.path.join(str(tmp_path), "monte_carlo_sobol.png")
    assert os.path.getsize(path) > 1000
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    assert path in capsys.readouterr().out
