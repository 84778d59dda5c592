"""plots.surrogate_figure from a hand-made result dict (no GPU, no library): the panels, the bars and the held-out scatter."""
import numpy as np

from erpl_monte_carlo_sim_amd import analysis, plots


def _result(validation=True):
    names = ["mass", "motor_thrust", "wind_speed", "wind_direction"]
    rng = np.random.default_rng(3)
    first = np.array([[0.5, 0.3, 0.05, 0.0], [0.1, 0.2, 0.3, np.nan]])
    total = np.array([[0.55, 0.35, 0.1, 0.05], [0.2, 0.3, 0.5, np.nan]])
    pair = np.zeros((2, 4, 4))
    pair[0, 0, 1] = pair[0, 1, 0] = 0.04
    pair[0, 2, 3] = pair[0, 3, 2] = 0.03
    pair[1, 0, 2] = pair[1, 2, 0] = 0.09
    pair[1, 1, 3] = pair[1, 3, 1] = np.nan
    out = {"names": names, "rows": [2, 4], "row_names": ["first_apogee_altitude", "range"], "first": first, "total": total, "pair": pair,
           "r2": np.array([0.97, 0.8]), "q2": np.array([0.96, np.nan]), "n_fit": 768, "n_val": 256, "degree": 2, "order": 2, "n_terms": 15}
    if validation:
        flown = rng.normal(size=(2, 256)) * 100.0 + 9000.0
        out["validation"] = {"samples": np.arange(256), "flown": flown, "predicted": flown + rng.normal(size=(2, 256))}
    return analysis.finish_polynomial_chaos(out, top=3)


def test_ranking_and_interactions_of_a_hand_made_result():
    out = _result()
    assert out["ranking"][0] == ["mass", "motor_thrust", "wind_speed", "wind_direction"]
    assert out["ranking"][1] == ["wind_speed", "motor_thrust", "mass", "wind_direction"]      # the NaN last
    assert out["interactions"][0][:2] == [("mass", "motor_thrust", 0.04), ("wind_speed", "wind_direction", 0.03)]
    assert len(out["interactions"][0]) == 3 and out["interactions"][1][0] == ("mass", "wind_speed", 0.09)
    assert all(np.isfinite(v) for _, _, v in out["interactions"][1])


def test_surrogate_figure_draws_three_panels_per_row(tmp_path):
    fig = plots.surrogate_figure(_result())
    axes = fig.get_axes()
    assert len(axes) == 6
    bars = [p for p in axes[0].patches]
    assert len(bars) == 8 and "r2 = 0.9700" in axes[0].get_title() and "768 fitted" in axes[0].get_title()
    assert [t.get_text() for t in axes[1].get_yticklabels()][0] == "mass x motor_thrust"
    assert len(axes[2].lines) == 2 and len(axes[2].lines[0].get_xdata()) == 256
    path = plots.save_figure(fig, str(tmp_path), "surrogate.png")
    assert open(path, "rb").read(4) == b"\x89PNG"


def test_surrogate_figure_without_held_out_members():
    fig = plots.surrogate_figure(_result(validation=False))
    assert not fig.get_axes()[2].axison and not fig.get_axes()[5].axison
