"""plots.debris_footprint_figure on a synthetic footprint dict (no GPU, no library): the two panels, one median line and
one band per fragment, the footprint boxes and the count grid at the chosen node, the keep-in outline and the file."""
import os

import numpy as np
import pytest

pytest.importorskip("matplotlib")

from erpl_monte_carlo_sim_amd import analysis, plots  # noqa: E402

Q = [0.05, 0.5, 0.95]
KEEP = [(-500.0, -500.0), (3000.0, -500.0), (3000.0, 500.0), (-500.0, 500.0)]
FRAGS = [(5.0, 30.0), (200.0, 10.0), (float("inf"), 0.0)]


def make_footprint(nodes=8, q=Q, keep=KEEP, frags=FRAGS, maps=((7, 1),), seed=4):
    rng = np.random.default_rng(seed)
    t = 5.0 * np.arange(nodes)
    F = len(frags)
    out = {"time": t, "q": list(q), "fragments": list(frags), "channels": list(analysis.DEBRIS_CHANNELS), "n_counted": 400,
           "keep_in": keep, "exit_probability": 0.25 if keep else float("nan"),
           "exit_interval": (0.21, 0.29) if keep else (0.0, 1.0), "maps": {}}
    clouds = {}
    for j, name in enumerate(analysis.DEBRIS_CHANNELS):
        cloud = (j + 1) * 10.0 * t[None, :, None] * (1.0 + np.arange(F))[None, None, :] + rng.normal(size=(400, nodes, F)) * 20.0
        cloud[:, 0, 0] = np.nan   # the lightest fragment of the first node never lands
        clouds[name] = cloud
        with np.errstate(all="ignore"):
            out[name] = {"count": np.sum(np.isfinite(cloud), axis=0), "mean": np.nanmean(cloud, axis=0),
                         "std": np.nanstd(cloud, axis=0), "min": np.nanmin(cloud, axis=0), "max": np.nanmax(cloud, axis=0),
                         "quantiles": np.nanquantile(cloud, q, axis=0) if len(q) else np.zeros((0, nodes, F))}
    for k, f in maps:
        counts, ex, ey = np.histogram2d(clouds["x"][:, k, f], clouds["y"][:, k, f], bins=12)
        out["maps"][(k, f)] = {"counts": counts.astype(np.int64), "edges_x": ex, "edges_y": ey, "info": {"counted": 400}}
    return out


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_figure_panels_lines_bands_boxes_and_outline():
    res = make_footprint()
    ax_r, ax_xy = plots.debris_footprint_figure(res).get_axes()
    assert ax_r.get_ylabel() == "Impact Range (m)" and "Break-up" in ax_r.get_xlabel()
    assert "25.00 %" in ax_r.get_title() and "[21.00, 29.00]" in ax_r.get_title() and "5 - 95 %" in ax_r.get_title()
    lines = ax_r.get_lines()
    assert len(lines) == 3 and len(ax_r.collections) == 3               # a median and a 5 - 95 % band per fragment
    for f, line in enumerate(lines):
        np.testing.assert_array_equal(line.get_xdata(), res["time"])
        np.testing.assert_array_equal(line.get_ydata(), res["range"]["quantiles"][1][:, f])
    labels = [t.get_text() for t in ax_r.get_legend().get_texts()]
    assert labels == ["beta 5 kg/m2, dv 30 m/s", "beta 200 kg/m2, dv 10 m/s", "beta inf kg/m2, dv 0 m/s"]
    # the footprint at the last node: per fragment a box and a centre mark, then the outline; one count grid
    xy = ax_xy.get_lines()
    assert len(xy) == 7 and len(ax_xy.collections) == 1
    box, mark = xy[2], xy[3]                                            # fragment 1
    xq, yq = res["x"]["quantiles"], res["y"]["quantiles"]
    assert list(box.get_xdata()) == [xq[0][7, 1], xq[2][7, 1], xq[2][7, 1], xq[0][7, 1], xq[0][7, 1]]
    assert list(box.get_ydata()) == [yq[0][7, 1], yq[0][7, 1], yq[2][7, 1], yq[2][7, 1], yq[0][7, 1]]
    assert list(mark.get_xdata()) == [xq[1][7, 1]] and list(mark.get_ydata()) == [yq[1][7, 1]]
    assert list(xy[-1].get_xdata()) == [-500.0, 3000.0, 3000.0, -500.0, -500.0]    # closed
    assert "400 samples" in ax_xy.get_title() and "35 s" in ax_xy.get_title()
    # another node: no map there; node 0 has no box for the fragment that never lands
    ax_r, ax_xy = plots.debris_footprint_figure(res, node=0).get_axes()
    assert len(ax_xy.collections) == 0 and len(ax_xy.get_lines()) == 5 and "at 0 s" in ax_xy.get_title()
    with pytest.raises(ValueError):
        plots.debris_footprint_figure(res, node=8)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_figure_without_polygon_or_quantiles():
    res = make_footprint(q=[], keep=None, maps=())
    ax_r, ax_xy = plots.debris_footprint_figure(res).get_axes()
    assert len(ax_r.collections) == 0 and len(ax_r.get_lines()) == 3 and len(ax_xy.get_lines()) == 3
    np.testing.assert_array_equal(ax_r.get_lines()[1].get_ydata(), res["range"]["mean"][:, 1])
    assert "%" not in ax_r.get_title() and ax_xy.get_legend() is None


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_plot_writes_the_file(tmp_path):
    class Analyzer:
        def _create_output_directory(self):
            return str(tmp_path)

    out = plots.plot_debris_footprint(Analyzer(), make_footprint(), None, True)
    assert out == str(tmp_path) and os.path.getsize(os.path.join(out, "monte_carlo_debris.png")) > 10000
    assert plots.plot_debris_footprint(Analyzer(), make_footprint(), 3, False) is None
