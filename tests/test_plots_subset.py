"""plots.rare_event_figure from a hand-made result dict (no GPU, no library calls): the curve on a log axis with its band, the
level thresholds, the estimate at the target, and a tally's exceedance drawn under it."""
import numpy as np

from erpl_monte_carlo_sim_amd import plots


def _result(target=4200.0):
    x = np.linspace(1000.0, 4500.0, 120)
    p = 10.0 ** (-(x - 1000.0) / 600.0)
    levels = [{"threshold": t, "p": 0.125, "delta": 0.02 * (i + 1), "gamma": 0.5 * i, "acceptance": None if i == 0 else 0.4, "n1": 512}
              for i, t in enumerate((1540.0, 2080.0, 2630.0, 3170.0))]
    return {"probability": 4.6e-6, "cov": 0.18, "interval": (3.2e-6, 6.6e-6), "interval_level": 0.95, "target": target, "reached": True,
            "levels": levels, "thresholds": [lv["threshold"] for lv in levels], "curve": np.column_stack([x, p]),
            "curve_cov": np.linspace(0.0, 0.18, 120), "evaluations": 25600, "row": "range", "tail": "upper"}


def _tally():
    edges = np.linspace(0.0, 5000.0, 51)
    counts = np.zeros(50, dtype=np.int64)
    counts[10:30] = np.arange(20, 0, -1) * 50
    return {"rows": {"range": {"count": int(counts.sum()) + 3, "above": 3, "histogram": {"edges": edges, "counts": counts}}}}


def test_rare_event_figure_draws_the_curve_its_band_and_the_levels(tmp_path):
    fig = plots.rare_event_figure(_result())
    ax, = fig.get_axes()
    assert ax.get_yscale() == "log" and ax.get_xlabel() == "range" and "4 levels" in ax.get_title() and "25600" in ax.get_title()
    curve = ax.lines[0]
    assert len(curve.get_xdata()) == 120 and curve.get_ydata()[0] == 1.0
    dashed = [ln for ln in ax.lines if ln.get_linestyle() == "--"]
    assert [ln.get_xdata()[0] for ln in dashed] == [1540.0, 2080.0, 2630.0, 3170.0]
    assert len(ax.collections) >= 1                                   # the band
    labels = [t.get_text() for t in ax.get_legend().get_texts()]
    assert "subset simulation" in labels and any(s.startswith("P = 4.6e-06") for s in labels) and "95 % band" in labels
    path = plots.save_figure(fig, str(tmp_path), "rare.png")
    assert open(path, "rb").read(4) == b"\x89PNG"


def test_rare_event_figure_over_a_tally_and_without_a_target():
    fig = plots.rare_event_figure(_result(target=None), tally=_tally())
    ax, = fig.get_axes()
    labels = [t.get_text() for t in ax.get_legend().get_texts()]
    assert any(s.startswith("direct Monte Carlo") for s in labels) and not any(s.startswith("P =") for s in labels)
    steps = ax.lines[0]
    count = _tally()["rows"]["range"]["count"]
    assert steps.get_ydata()[0] == 1.0 and len(steps.get_xdata()) == 51 and steps.get_ydata()[-1] == 3 / count   # the mass above the range
    lower = dict(_result(), tail="lower")
    assert plots.rare_event_figure(lower).get_axes()[0].get_xlabel() == "-range"
