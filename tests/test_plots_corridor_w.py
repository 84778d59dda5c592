"""plots.reweighted_corridor_figure / plot_reweighted_corridor on a hand-made dict of analysis.reweighted_corridor (no GPU, no
library): the panels, flown bands dashed and reweighted bands solid, the per-node effective sample size on a second axis, and
the JSON file next to the figure."""
import json
import os

import numpy as np
import pytest

pytest.importorskip("matplotlib")

from erpl_monte_carlo_sim_amd import plots  # noqa: E402

Q = [0.05, 0.5, 0.95]


def make_result():
    t = np.linspace(0.0, 20.0, 9)
    out = {"time": t, "channels": ["z", "downrange"], "q": list(Q), "thresholds": [[100.0], []], "m": 400, "n_masked": 12,
           "n_counted": 388, "max_w": 1 << 52, "K": 53, "Q": 52, "ess": 61.5, "ess_expected_share": 0.13, "n_outside": 200,
           "sum_w": 123456789, "ess_share": 0.16, "max_weight_share": 0.05, "warnings": ["the effective sample size is 61.5, below 100"]}
    for k, name in enumerate(out["channels"]):
        base = (k + 1) * 100.0 * np.sin(t / 7.0)
        flown = {"count": np.full(9, 388), "mean": base, "std": np.full(9, 10.0), "min": base - 30, "max": base + 30,
                 "quantiles": np.stack([base - 16, base, base + 16])}
        rew = {"count": np.full(9, 188), "mean": base + 5, "mean_se": np.full(9, 1.5), "std": np.full(9, 8.0), "min": base - 25,
               "max": base + 28, "ess": np.linspace(60.0, 20.0, 9), "sum_w": np.full(9, 123456789, dtype=np.int64),
               "quantiles": np.stack([base - 9, base + 5, base + 19]), "p": np.full((1 - k, 9), 0.25), "p_se": np.full((1 - k, 9), 0.03),
               "exceed_w": np.full((1 - k, 9), 30864197, dtype=np.int64)}
        out[name] = {"reweighted": rew, "flown": flown}
    return out


def test_figure_draws_flown_dashed_reweighted_solid_and_the_ess():
    res = make_result()
    fig = plots.reweighted_corridor_figure(res)
    axes = fig.get_axes()
    assert len(axes) == 4   # a panel and its twin per channel
    panels = [ax for ax in axes if ax.get_ylabel() in ("Altitude (m)", "Downrange (m)")]
    twins = [ax for ax in axes if ax.get_ylabel() == "Effective samples"]
    assert len(panels) == 2 and len(twins) == 2 and panels[-1].get_xlabel() == "Time (s)"
    assert "388 samples" in panels[0].get_title() and "effective 62" in panels[0].get_title()
    for ax, twin, name in zip(panels, twins, res["channels"]):
        lines = ax.get_lines()
        assert len(lines) == 6
        dashed = [ln for ln in lines if ln.get_linestyle() == "--"]
        solid = [ln for ln in lines if ln.get_linestyle() == "-"]
        assert len(dashed) == 3 and len(solid) == 3
        want_flown = {tuple(row) for row in res[name]["flown"]["quantiles"]}
        want_rew = {tuple(row) for row in res[name]["reweighted"]["quantiles"]}
        assert {tuple(ln.get_ydata()) for ln in dashed} == want_flown and {tuple(ln.get_ydata()) for ln in solid} == want_rew
        (ess,) = twin.get_lines()
        np.testing.assert_array_equal(ess.get_ydata(), res[name]["reweighted"]["ess"])
    labels = [t.get_text() for t in panels[0].get_legend().get_texts()]
    assert "flown 50 %" in labels and "reweighted 50 %" in labels and "reweighted 5 - 95 %" in labels


def test_figure_without_quantiles_draws_the_means():
    res = make_result()
    res["q"] = []
    for name in res["channels"]:
        res[name]["flown"]["quantiles"] = np.zeros((0, 9))
        res[name]["reweighted"]["quantiles"] = np.zeros((0, 9))
    fig = plots.reweighted_corridor_figure(res)
    ax = [a for a in fig.get_axes() if a.get_ylabel() == "Altitude (m)"][0]
    assert [ln.get_label() for ln in ax.get_lines()] == ["flown mean", "reweighted mean"]


def test_plot_writes_the_figure_and_the_json(tmp_path):
    class Analyzer:
        def _create_output_directory(self):
            return str(tmp_path)

    res = make_result()
    out = plots.plot_reweighted_corridor(Analyzer(), res)
    assert out == str(tmp_path) and os.path.getsize(os.path.join(out, "monte_carlo_reweighted_corridor.png")) > 0
    with open(os.path.join(out, "reweighted_corridor.json")) as fh:
        back = json.load(fh)
    assert back["channels"] == ["z", "downrange"] and back["max_w"] == 1 << 52 and back["warnings"] == res["warnings"]
    assert back["z"]["reweighted"]["ess"] == list(res["z"]["reweighted"]["ess"])
    assert back["z"]["flown"]["quantiles"][1] == list(res["z"]["flown"]["quantiles"][1])
    assert plots.plot_reweighted_corridor(Analyzer(), res, save_plots=False) is None
