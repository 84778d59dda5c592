"""plots.run_comparison_figure on a result made by hand (no GPU, no library): the panels, their labels, the distribution
functions with the Kolmogorov-Smirnov location, the shift function, the null histograms, the clouds, and the file."""
import os

import numpy as np
import pytest

pytest.importorskip("matplotlib")

from erpl_monte_carlo_sim_amd import analysis, plots  # noqa: E402


def a_test(stat, p, P):
    exceed = int(round(p * (P + 1))) - 1 if P else 0
    return {"statistic": stat, "p_value": p if P else float("nan"), "null_mean": 0.5 * stat if P else float("nan"),
            "null_hi": 0.8 * stat if P else float("nan"), "exceed": exceed}


def make_comparison(P=199, keep_null=True, bivariate=True, seed=2):
    """A hand-made dict of TrajectoryEngine.compare over apogee and range, finished by analysis.finish_comparison as
    compare_runs does: apogee alike, range moved."""
    rng = np.random.default_rng(seed)
    levels = np.linspace(0.0, 1.0, 64)
    q = [0.05, 0.25, 0.5, 0.75, 0.95]
    a = np.sort(rng.normal(size=(2, 64)), axis=1)
    b = np.sort(rng.normal(size=(2, 64)), axis=1) + np.array([[0.0], [0.8]])
    rows = []
    for j, p in enumerate((0.6, 1.0 / (P + 1) if P else float("nan"))):
        qa, qb = np.quantile(a[j], q), np.quantile(b[j], q)
        rows.append({"mean_a": a[j].mean(), "std_a": a[j].std(), "mean_b": b[j].mean(), "std_b": b[j].std(),
                     "quantile_a": list(qa), "quantile_b": list(qb), "shift": list(qb - qa), "ks_num": 1200 + 9000 * j,
                     "u2_a": 30000, "ks_at": float(a[j][32]), "ks_sign": 1, "prob_superiority": 0.5 - 0.2 * j,
                     "ks": a_test(0.05 + 0.3 * j, p, P), "mw": a_test(800.0, p, P), "cvm": a_test(0.2 + 3 * j, p, P)})
    out = {"n_a": 400, "n_b": 300, "count_a": 320, "count_b": 250, "rows": [0, 4], "q": q, "xy": (8, 9) if bivariate else None,
           "permutations": P, "level": 0.95, "seed": 0, "row": rows, "ecdf": {"levels": levels, "a": a, "b": b},
           "energy": dict(a_test(0.06, 1.0 / (P + 1) if P else float("nan"), P), d_ab=1.9, d_aa=1.8, d_bb=1.85) if bivariate else None}
    if bivariate:
        out["cloud_a"] = {"mean": np.array([10.0, -5.0]), "cov": np.array([[4.0, 1.5], [1.5, 2.0]])}
        out["cloud_b"] = {"mean": np.array([11.0, -5.5]), "cov": np.array([[4.0, -1.5], [-1.5, 2.0]])}
    if keep_null and P:
        out["null_values"] = np.abs(rng.normal(size=(7, P))) * np.array([[1000.0], [1.0], [1.0], [1000.0], [1.0], [1.0], [0.01]])
    return analysis.finish_comparison(out)


def test_finish_adds_names_p_values_and_verdicts():
    out = make_comparison()
    assert [r["name"] for r in out["row"]] == ["apogee_altitude", "range"]
    assert out["row"][0]["p_values"] == {"ks": 0.6, "mw": 0.6, "cvm": 0.6}
    assert "no difference at 0.05" in out["row"][0]["verdict"] and "smallest p = 0.6" in out["row"][0]["verdict"]
    v = out["row"][1]["verdict"]
    assert v.startswith("range: differs at 0.05") and "Kolmogorov-Smirnov" in v and "Mann-Whitney" in v and "Cramer-von Mises" in v
    assert "P(A > B) = 0.300" in v and "mean shift +" in v
    assert out["energy_verdict"].startswith("impact clouds: differ at 0.05") and "p = 0.005" in out["energy_verdict"]
    bare = make_comparison(P=0, bivariate=False)
    assert all("not tested" in r["verdict"] for r in bare["row"]) and bare["energy_verdict"] == "impact clouds: not tested"
    extra = make_comparison()
    extra["rows"] = [0, 16]
    assert analysis.finish_comparison(extra)["row"][1]["name"] == "extra"


def test_run_comparison_figure_panels_and_labels():
    out = make_comparison()
    fig = plots.run_comparison_figure(out)
    axes = fig.get_axes()
    assert len(axes) == 9                                                    # per row three panels, and the row of the clouds
    assert "199 permutations" in fig._suptitle.get_text() and "0.95" in fig._suptitle.get_text()
    for j, name in enumerate(("apogee_altitude", "range")):
        ecdf_ax, shift_ax, null_ax = axes[3 * j:3 * j + 3]
        assert ecdf_ax.get_title() == f"{name}: distribution functions" and ecdf_ax.get_ylabel() == "F"
        steps = [ln for ln in ecdf_ax.get_lines() if ln.get_label().startswith(("A (", "B ("))]
        assert [ln.get_label() for ln in steps] == ["A (320)", "B (250)"]
        np.testing.assert_array_equal(steps[0].get_xdata(), out["ecdf"]["a"][j])
        np.testing.assert_array_equal(steps[1].get_xdata(), out["ecdf"]["b"][j])
        np.testing.assert_array_equal(steps[0].get_ydata(), out["ecdf"]["levels"])
        marks = [ln for ln in ecdf_ax.get_lines() if ln.get_label().startswith("D = ")]
        assert len(marks) == 1 and marks[0].get_xdata()[0] == out["row"][j]["ks_at"]
        (line,) = shift_ax.get_lines()[:1]
        np.testing.assert_array_equal(line.get_ydata(), out["row"][j]["shift"])
        np.testing.assert_array_equal(line.get_xdata(), out["q"])
        assert shift_ax.get_xlabel() == "quantile" and "shift function" in shift_ax.get_title()
        assert "null of K" in null_ax.get_title() and "p(ks)" in null_ax.get_title()
        assert sum(p.get_height() for p in null_ax.patches) == 199           # the histogram holds every null value
        assert [ln.get_xdata()[0] for ln in null_ax.get_lines()] == [out["row"][j]["ks_num"]]
    cloud_ax, dist_ax, e_ax = axes[6:]
    assert "E = 0.06" in cloud_ax.get_title() and "p = 0.005" in cloud_ax.get_title()
    assert (cloud_ax.get_xlabel(), cloud_ax.get_ylabel()) == ("impact x", "impact y")
    assert [t.get_text() for t in cloud_ax.get_legend().get_texts()] == ["A", "B"]
    assert [p.get_height() for p in dist_ax.patches] == [1.8, 1.9, 1.85]
    assert e_ax.get_title() == "null of E" and sum(p.get_height() for p in e_ax.patches) == 199


def test_figure_without_nulls_or_clouds_and_the_file(tmp_path):
    out = make_comparison(keep_null=False, bivariate=False)
    fig = plots.run_comparison_figure(out)
    axes = fig.get_axes()
    assert len(axes) == 6
    assert out["row"][1]["verdict"] in [t.get_text() for t in axes[5].texts] and not axes[5].patches
    empty = make_comparison(P=0, bivariate=False)
    assert len(plots.run_comparison_figure(empty).get_axes()) == 6

    class Analyzer:
        def _create_output_directory(self):
            return str(tmp_path)

    assert plots.plot_run_comparison(Analyzer(), make_comparison(), save_plots=True) == str(tmp_path)
    path = os.path.join(str(tmp_path), "monte_carlo_run_comparison.png")
    assert os.path.getsize(path) > 10000
    assert plots.plot_run_comparison(Analyzer(), make_comparison(), save_plots=False) is None
