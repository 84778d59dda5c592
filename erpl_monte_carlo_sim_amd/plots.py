"""Pictures of a Monte Carlo run: `plot_results`, `plot_trajectory_cloud` and `plot_trajectory_cloud_3d` of the reference
(monte_carlo.py:562-707: same panels, titles, axis labels and file names) plus the landing dispersion, in two layers.

Drawing functions take host data only - bin edges and counts, scatter points or a 2-D count grid, the dispersion dict,
trajectories - and build `matplotlib.figure.Figure` objects directly: no pyplot state, no `plt.show`, no change of the
global backend.  matplotlib is imported inside them, so the package imports without it.

The `plot_*` functions behind the MonteCarloAnalyzer methods get that data from the device: the histograms are counted by
erpl_mc_histogram over the samples the outlier filter keeps (the bars drawn over the device edges are what
`ax.hist(values, bins=50)` draws), the fourth panel scatters the points as the reference does up to SCATTER_MAX valid
samples and shows the erpl_mc_histogram_xy density above that, the landing picture comes from erpl_mc_histogram_xy and
erpl_mc_dispersion.  No per-sample dicts are built for any of it.
"""
import json
import math
import os

import numpy as np

from . import _abi

DPI = 300                 # monte_carlo.py:610
SCATTER_MAX = 20000       # valid samples up to which the range-vs-apogee panel is a scatter plot, as the reference's
DENSITY_BINS = 200        # bins per axis of the density that replaces it
LANDING_BINS = 100        # bins per axis of the impact footprint

HIST_PANELS = (("Apogee Altitude (m)", "Apogee Altitude Distribution"),
               ("Range (m)", "Range Distribution"),
               ("Flight Time (s)", "Flight Time Distribution"))


def _figure(figsize):
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    fig = Figure(figsize=figsize)
    FigureCanvasAgg(fig)
    return fig


def _density(ax, counts, edges_x, edges_y, cmap="viridis"):
    """A [bins_x, bins_y] count grid (x-major, as np.histogram2d) as an image; empty cells stay blank."""
    grid = np.ma.masked_equal(np.asarray(counts).T, 0)
    return ax.pcolormesh(np.asarray(edges_x), np.asarray(edges_y), grid, cmap=cmap, shading="flat")


# ---------------------------------------------------------------------------------------------- drawing layer
def distributions_figure(histograms, points=None, density=None):
    """The four panels of `plot_results` (monte_carlo.py:565-604).  histograms: three (edges, counts) pairs for apogee,
    range and flight time; fourth panel: points = (apogee, range) arrays to scatter, or density = (counts [bx, by],
    edges_x, edges_y) of the same pair."""
    fig = _figure((12, 10))
    axes = fig.subplots(2, 2)
    for ax, (edges, counts), (xlabel, title) in zip((axes[0, 0], axes[0, 1], axes[1, 0]), histograms, HIST_PANELS):
        edges, counts = np.asarray(edges, dtype=np.float64), np.asarray(counts)
        ax.bar(edges[:-1], counts, width=np.diff(edges), align="edge", alpha=0.7, edgecolor="black")
        ax.set_xlabel(xlabel)
        ax.set_ylabel("Frequency")
        ax.set_title(title)
        ax.grid(True, alpha=0.3)
    ax = axes[1, 1]
    if density is not None:
        fig.colorbar(_density(ax, *density), ax=ax, label="Samples per cell")
    elif points is not None:
        ax.scatter(np.asarray(points[0]), np.asarray(points[1]), alpha=0.6, s=10)
    ax.set_xlabel("Apogee Altitude (m)")
    ax.set_ylabel("Range (m)")
    ax.set_title("Range vs Apogee Altitude")
    ax.grid(True, alpha=0.3)
    fig.tight_layout()
    return fig


def trajectory_cloud_figure(trajectories):
    """monte_carlo.py:635-668.  trajectories: result dicts; those with a 'trajectory' are drawn."""
    fig = _figure((15, 6))
    ax1, ax2 = fig.subplots(1, 2)
    for result in trajectories:
        if "trajectory" in result:
            ax1.plot(result["trajectory"]["time"], result["trajectory"]["altitude"], alpha=0.3, linewidth=0.5, color="blue")
    ax1.set_xlabel("Time (s)")
    ax1.set_ylabel("Altitude (m)")
    ax1.set_title(f"Trajectory Cloud - Altitude vs Time\n({len(trajectories)} trajectories)")
    ax1.grid(True, alpha=0.3)
    for result in trajectories:
        if "trajectory" in result and "position" in result["trajectory"]:
            pos = np.asarray(result["trajectory"]["position"])
            ax2.plot(pos[:, 0], pos[:, 1], alpha=0.3, linewidth=0.5, color="red")
    ax2.set_xlabel("East Position (m)")
    ax2.set_ylabel("North Position (m)")
    ax2.set_title(f"Ground Track Cloud\n({len(trajectories)} trajectories)")
    ax2.grid(True, alpha=0.3)
    ax2.axis("equal")
    fig.tight_layout()
    return fig


def trajectory_cloud_3d_figure(trajectories):
    """monte_carlo.py:679-699."""
    from mpl_toolkits.mplot3d import Axes3D  # noqa: F401  (registers the projection on older matplotlib)
    fig = _figure((10, 8))
    ax = fig.add_subplot(111, projection="3d")
    for result in trajectories:
        if "trajectory" in result and "position" in result["trajectory"]:
            pos = np.asarray(result["trajectory"]["position"])
            ax.plot(pos[:, 0], pos[:, 1], pos[:, 2], alpha=0.3, linewidth=0.5)
    ax.set_xlabel("East Position (m)")
    ax.set_ylabel("North Position (m)")
    ax.set_zlabel("Altitude (m)")
    ax.set_title(f"3D Trajectory Cloud ({len(trajectories)} trajectories)")
    ax.grid(True, alpha=0.3)
    return fig


def landing_figure(dispersion, density=None, points=None):
    """Impact footprint: density = (counts [bx, by], edges_x, edges_y) of the impact point or points = (x, y) to scatter,
    the confidence ellipses of the dispersion dict (TrajectoryEngine.dispersion: centred on 'mean', full axes
    2 * semi_major by 2 * semi_minor, turned by 'angle') and the CEP circle about 'centre'."""
    from matplotlib.patches import Circle, Ellipse
    fig = _figure((9, 8))
    ax = fig.subplots()
    if density is not None:
        fig.colorbar(_density(ax, *density, cmap="Greys"), ax=ax, label="Samples per cell")
    elif points is not None:
        ax.scatter(np.asarray(points[0]), np.asarray(points[1]), alpha=0.4, s=6, color="grey")
    mean, centre = dispersion["mean"], dispersion["centre"]
    colours = ("tab:green", "tab:orange", "tab:red", "tab:purple", "tab:brown", "tab:pink", "tab:olive", "tab:cyan")
    for k, e in enumerate(dispersion["ellipses"]):
        if not (np.isfinite(e["semi_major"]) and np.isfinite(e["semi_minor"])):
            continue
        share = f", holds {e['inside']} of {dispersion['count']}" if e["inside"] >= 0 else ""
        ax.add_patch(Ellipse(xy=(mean[0], mean[1]), width=2 * e["semi_major"], height=2 * e["semi_minor"],
                             angle=math.degrees(dispersion["angle"]), fill=False, linewidth=1.5,
                             edgecolor=colours[k % len(colours)], label=f"{100 * e['level']:g} % ellipse{share}"))
    cep = dispersion.get("cep")
    if cep is not None and np.isfinite(cep):
        ax.add_patch(Circle((centre[0], centre[1]), cep, fill=False, linestyle="--", linewidth=1.5, edgecolor="tab:blue",
                            label=f"CEP {cep:.1f} m"))
        ax.plot([centre[0]], [centre[1]], marker="+", color="tab:blue", markersize=10)
    if np.isfinite(mean[0]) and np.isfinite(mean[1]):
        ax.plot([mean[0]], [mean[1]], marker="x", color="black", markersize=8)
    ax.set_xlabel("East Position (m)")
    ax.set_ylabel("North Position (m)")
    ax.set_title(f"Landing Dispersion ({dispersion['count']} impacts)")
    ax.grid(True, alpha=0.3)
    ax.set_aspect("equal", adjustable="datalim")
    ax.autoscale_view()
    if ax.get_legend_handles_labels()[0]:
        ax.legend(loc="best", fontsize=8)
    fig.tight_layout()
    return fig


def drivers_figure(drivers, row, top=10):
    """Tornado chart of one outcome: horizontal bars of `spearman` and `srrc` (pearson and src for a dict computed with
    ranks=False) of its `top` strongest factors, strongest on top, R^2 of the (rank) regression in the title.  drivers:
    the dict of analysis.drivers; row: an index into its rows or one of its row_names."""
    j = drivers["row_names"].index(row) if isinstance(row, str) else int(row)
    ranked = drivers["rank_corr"] is not None
    rho = np.asarray(drivers["spearman" if ranked else "pearson"])[j]
    beta = np.asarray(drivers["srrc" if ranked else "src"])[j]
    r2 = float(np.asarray(drivers["r2_rank" if ranked else "r2"])[j])
    names = list(drivers["factor_names"])
    order = [names.index(k) for k in drivers["ranking"][j] if not np.isnan(rho[names.index(k)])][:int(top)]
    fig = _figure((9, 0.45 * max(len(order), 1) + 2.0))
    ax = fig.subplots()
    y = np.arange(len(order))[::-1].astype(np.float64)
    ax.barh(y + 0.2, rho[order], height=0.4, label="Spearman" if ranked else "Pearson", alpha=0.8, edgecolor="black")
    ax.barh(y - 0.2, np.nan_to_num(beta[order]), height=0.4, label="SRRC" if ranked else "SRC", alpha=0.8,
            edgecolor="black")
    ax.set_yticks(y)
    ax.set_yticklabels([names[f] for f in order])
    ax.axvline(0.0, color="black", linewidth=0.8)
    ax.set_xlim(-1.05, 1.05)
    ax.set_xlabel("Rank correlation / standardised rank regression coefficient" if ranked
                  else "Correlation / standardised regression coefficient")
    fit = "regression singular" if np.isnan(r2) else f"R\u00b2 = {r2:.3f}"
    ax.set_title(f"Drivers of {drivers['row_names'][j]} ({fit}, {drivers['count']} samples)")
    ax.grid(True, axis="x", alpha=0.3)
    ax.legend(loc="lower right")
    fig.tight_layout()
    return fig


def impact_probability_figure(result, launch_site=(0.0, 0.0)):
    """The impact probability map from the dict of analysis.impact_probability: filled contours of the density between its
    thresholds (the band down to thresholds[k] is the region that holds levels[k] of the landings; the widest region is
    drawn first), each labelled with its content, the outline of every zone labelled with its probability, the launch site
    marked.  A result that is not solid draws the zones and the launch site only."""
    from matplotlib.patches import Patch, Polygon
    fig = _figure((9, 8))
    ax = fig.subplots()
    handles = []
    pairs = sorted((t, p) for t, p in zip(result["thresholds"], result["levels"]) if np.isfinite(t) and t > 0.0)
    cuts, contents = [], []
    for t, p in pairs:   # ascending thresholds = descending content; equal thresholds keep the first
        if not cuts or t > cuts[-1]:
            cuts.append(t)
            contents.append(p)
    if result["solid"] and cuts:
        dens = np.asarray(result["density"], dtype=np.float64)
        top = max(float(np.max(dens)), cuts[-1]) * (1.0 + 1e-9) + np.finfo(np.float64).tiny
        shades = [str(0.85 - 0.6 * k / max(len(cuts) - 1, 1)) for k in range(len(cuts))]
        ax.contourf(np.asarray(result["grid_x"]), np.asarray(result["grid_y"]), dens.T, levels=cuts + [top], colors=shades)
        ax.contour(np.asarray(result["grid_x"]), np.asarray(result["grid_y"]), dens.T, levels=cuts, colors="black",
                   linewidths=0.6)
        handles += [Patch(facecolor=c, edgecolor="black", label=f"{100 * p:g} % of landings") for c, p in zip(shades, contents)]
    colours = ("tab:red", "tab:blue", "tab:green", "tab:orange", "tab:purple", "tab:brown", "tab:pink", "tab:olive")
    for k, z in enumerate(result["zones"]):
        label = f"zone {k}: {z['inside']} of {result['count']}"
        if "probability" in z and np.isfinite(z["probability"]):
            label = f"zone {k}: P = {z['probability']:.4g} [{z['interval'][0]:.4g}, {z['interval'][1]:.4g}]"
        patch = Polygon(np.asarray(z["vertices"], dtype=np.float64), closed=True, fill=False, linewidth=1.5,
                        edgecolor=colours[k % len(colours)], label=label)
        ax.add_patch(patch)
        handles.append(patch)
    if launch_site is not None:
        handles += ax.plot([launch_site[0]], [launch_site[1]], marker="*", color="black", markersize=12, linestyle="none",
                           label="Launch site")
    (lo_x, hi_x), (lo_y, hi_y) = result["ranges"]
    if np.isfinite([lo_x, hi_x, lo_y, hi_y]).all():
        ax.update_datalim([(lo_x, lo_y), (hi_x, hi_y)])
    ax.set_xlabel("East Position (m)")
    ax.set_ylabel("North Position (m)")
    ax.set_title(f"Impact Probability ({result['count']} impacts)")
    ax.grid(True, alpha=0.3)
    ax.set_aspect("equal", adjustable="datalim")
    ax.autoscale_view()
    if handles:
        ax.legend(handles=handles, loc="best", fontsize=8)
    fig.tight_layout()
    return fig


def reweighted_impact_figure(result, launch_site=(0.0, 0.0)):
    """The weighted impact probability map from the dict of analysis.reweighted_impact, drawn by `impact_probability_figure`
    (the zones carry 'probability' and 'interval' = probability -+ 1.96 se), titled with the effective sample size."""
    view = dict(result)
    view["zones"] = [dict(z, inside=z["weight"]) for z in result["zones"]]
    fig = impact_probability_figure(view, launch_site)
    ess = result.get("ess", float("nan"))
    fig.axes[0].set_title(f"Impact Probability under the target law ({result['count']} impacts, effective {ess:.0f})")
    return fig


CORRIDOR_LABELS = {"x": "x (m)", "y": "y (m)", "z": "Altitude (m)", "downrange": "Downrange (m)", "vx": "vx (m/s)",
                   "vy": "vy (m/s)", "vz": "vz (m/s)", "speed": "Speed (m/s)"}


def corridor_figure(result):
    """The flight corridor from the dict of analysis.trajectory_corridor: one panel per channel over time - the median line
    (the quantile nearest 0.5), the band between the outermost pair of quantiles and, with four or more quantiles, the band
    between the next pair inside it - and the number of samples behind every node on a twin axis."""
    names = list(result["channels"])
    q = np.asarray(result["q"], dtype=np.float64)
    t = np.asarray(result["time"], dtype=np.float64)
    fig = _figure((10, 3.2 * len(names) + 0.6))
    axes = np.atleast_1d(fig.subplots(len(names), 1, sharex=True))
    order = np.argsort(q)
    mid = int(np.argmin(np.abs(q - 0.5))) if len(q) else None
    for ax, name in zip(axes, names):
        ch = result[name]
        quant = np.asarray(ch["quantiles"], dtype=np.float64)
        for depth, alpha in ((0, 0.2), (1, 0.35)):   # the outer pair, then the inner one
            if len(q) >= 2 * (depth + 1):
                lo, hi = order[depth], order[len(q) - 1 - depth]
                ax.fill_between(t, quant[lo], quant[hi], alpha=alpha, color="tab:blue", linewidth=0,
                                label=f"{100 * q[lo]:g} - {100 * q[hi]:g} %")
        if mid is not None:
            ax.plot(t, quant[mid], color="tab:blue", linewidth=1.5, label=f"{100 * q[mid]:g} %")
        else:
            ax.plot(t, np.asarray(ch["mean"], dtype=np.float64), color="tab:blue", linewidth=1.5, label="mean")
        ax.set_ylabel(CORRIDOR_LABELS.get(name, name))
        ax.grid(True, alpha=0.3)
        twin = ax.twinx()
        twin.plot(t, np.asarray(ch["count"]), color="gray", linewidth=0.8, linestyle=":")
        twin.set_ylabel("Samples")
        twin.set_ylim(bottom=0)
    axes[0].set_title(f"Trajectory Corridor ({int(result.get('n_counted', 0))} samples)")
    axes[0].legend(loc="best", fontsize=8)
    axes[-1].set_xlabel("Time (s)")
    fig.tight_layout()
    return fig


def reweighted_corridor_figure(result):
    """The corridor under another input law from the dict of analysis.reweighted_corridor: one panel per channel over time -
    the flown bands dashed (the outermost pair of quantiles and the one nearest 0.5), the reweighted bands solid with the
    band between the outermost pair filled - and the effective sample size behind every node on a twin axis."""
    names = list(result["channels"])
    q = np.asarray(result["q"], dtype=np.float64)
    t = np.asarray(result["time"], dtype=np.float64)
    fig = _figure((10, 3.2 * len(names) + 0.6))
    axes = np.atleast_1d(fig.subplots(len(names), 1, sharex=True))
    order = np.argsort(q)
    mid = int(np.argmin(np.abs(q - 0.5))) if len(q) else None
    for ax, name in zip(axes, names):
        rew, flown = result[name]["reweighted"], result[name]["flown"]
        qr = np.asarray(rew["quantiles"], dtype=np.float64)
        qf = np.asarray(flown["quantiles"], dtype=np.float64)
        if len(q) >= 2:
            lo, hi = order[0], order[-1]
            ax.fill_between(t, qr[lo], qr[hi], alpha=0.2, color="tab:red", linewidth=0)
            for k in (lo, hi):
                ax.plot(t, qf[k], color="tab:blue", linewidth=1.0, linestyle="--",
                        label=f"flown {100 * q[lo]:g} - {100 * q[hi]:g} %" if k == lo else None)
                ax.plot(t, qr[k], color="tab:red", linewidth=1.0,
                        label=f"reweighted {100 * q[lo]:g} - {100 * q[hi]:g} %" if k == lo else None)
        if mid is not None:
            ax.plot(t, qf[mid], color="tab:blue", linewidth=1.5, linestyle="--", label=f"flown {100 * q[mid]:g} %")
            ax.plot(t, qr[mid], color="tab:red", linewidth=1.5, label=f"reweighted {100 * q[mid]:g} %")
        else:
            ax.plot(t, np.asarray(flown["mean"], dtype=np.float64), color="tab:blue", linewidth=1.5, linestyle="--", label="flown mean")
            ax.plot(t, np.asarray(rew["mean"], dtype=np.float64), color="tab:red", linewidth=1.5, label="reweighted mean")
        ax.set_ylabel(CORRIDOR_LABELS.get(name, name))
        ax.grid(True, alpha=0.3)
        twin = ax.twinx()
        twin.plot(t, np.asarray(rew["ess"], dtype=np.float64), color="gray", linewidth=0.8, linestyle=":")
        twin.set_ylabel("Effective samples")
        twin.set_ylim(bottom=0)
    ess = result.get("ess", float("nan"))
    axes[0].set_title(f"Trajectory Corridor under the target law ({int(result.get('n_counted', 0))} samples, effective {ess:.0f})")
    axes[0].legend(loc="best", fontsize=8)
    axes[-1].set_xlabel("Time (s)")
    fig.tight_layout()
    return fig


def corridor_drivers_figure(result, top=4):
    """Which dispersion drives what, and when, from the dict of analysis.corridor_drivers: per channel two panels over time -
    the signed correlation of the `top` factors of the channel's ranking, and under it their stacked linear variance shares
    (pearson^2, the remaining factors as 'others') with r2 of the standardised regression as the outline.  A node without a
    number leaves a gap."""
    names = list(result["channels"])
    t = np.arange(len(result["time"]), dtype=np.float64) if "fragments" in result else np.asarray(result["time"], dtype=np.float64)
    pearson = np.asarray(result["pearson"], dtype=np.float64)
    share = np.nan_to_num(np.asarray(result["share"], dtype=np.float64), nan=0.0)
    r2 = np.asarray(result["r2"], dtype=np.float64)
    factor_names = list(result["factor_names"])
    fig = _figure((10, 4.4 * len(names) + 0.6))
    axes = np.atleast_2d(fig.subplots(2 * len(names), 1, sharex=True).reshape(len(names), 2)) if len(names) else []
    for c, name in enumerate(names):
        ax, bx = axes[c]
        lead = [factor_names.index(n) for n in result["ranking"][c][:max(1, int(top))]]
        for f in lead:
            ax.plot(t, pearson[c, :, f], linewidth=1.3, label=factor_names[f])
        ax.axhline(0.0, color="gray", linewidth=0.6)
        ax.set_ylim(-1.05, 1.05)
        ax.set_ylabel(f"{CORRIDOR_LABELS.get(name, name)}\ncorrelation")
        ax.grid(True, alpha=0.3)
        ax.legend(loc="best", fontsize=7, ncol=2)
        rest = [f for f in range(len(factor_names)) if f not in lead]
        stacks = [share[c, :, f] for f in lead] + ([share[c][:, rest].sum(axis=1)] if rest else [])
        bx.stackplot(t, *stacks, labels=[factor_names[f] for f in lead] + (["others"] if rest else []), alpha=0.7)
        if np.any(np.isfinite(r2[c])):
            bx.plot(t, r2[c], color="black", linewidth=1.2, label="r2")
        bx.set_ylabel("variance share")
        bx.set_ylim(bottom=0.0)
        bx.grid(True, alpha=0.3)
    if len(names):
        axes[0][0].set_title(f"Corridor Drivers ({int(result.get('n_base', 0))} samples)")
        axes[-1][1].legend(loc="best", fontsize=7, ncol=2)
        axes[-1][1].set_xlabel("Row (node, fragment)" if "fragments" in result else "Time (s)")
    fig.tight_layout()
    return fig


def functional_boxplot_figure(result, values=None, most=20):
    """The functional boxplot (Sun & Genton 2011) from the dict of analysis.trajectory_depth: per channel the central region
    as a band, the median flight - a flight that was flown - as a line, the whiskers (the envelope of the flights that never
    leave the fences) and, with `values` (the [C, T, ld] matrix the depth was taken of, a tensor or an array), up to `most`
    of the magnitude outliers (red) and of the shape outliers (orange) drawn one by one."""
    names = list(result["channels"])
    t = np.arange(len(result["time"]), dtype=np.float64) if "fragments" in result else np.asarray(result["time"], dtype=np.float64)
    fig = _figure((10, 3.4 * len(names) + 0.6))
    axes = np.atleast_1d(fig.subplots(len(names), 1, sharex=True)) if len(names) else []
    for c, name in enumerate(names):
        ax, ch = axes[c], result[name]
        ax.fill_between(t, ch["central"]["lo"], ch["central"]["hi"], color="tab:blue", alpha=0.35,
                        label=f"central {100.0 * result['central_share']:.0f} %")
        ax.plot(t, ch["whisker"]["lo"], color="tab:blue", linewidth=0.9, label="whiskers")
        ax.plot(t, ch["whisker"]["hi"], color="tab:blue", linewidth=0.9)
        drawn = 0
        if values is not None:
            for key, colour in (("magnitude_outliers", "tab:red"), ("shape_outliers", "tab:orange")):
                cols = [o["column"] if isinstance(o, dict) else o for o in (ch[key] or [])][:max(0, int(most))]
                for i, j in enumerate(cols):
                    col = values[c, :, j]
                    col = col.cpu().numpy() if hasattr(col, "cpu") else np.asarray(col)
                    ax.plot(t, col, color=colour, linewidth=0.7, alpha=0.8, label=key.replace("_", " ") if i == 0 else None)
                    drawn += 1
        ax.plot(t, ch["median_curve"], color="black", linewidth=1.4, label=f"median flight (sample {ch['median']})")
        ax.set_ylabel(CORRIDOR_LABELS.get(name, name))
        ax.grid(True, alpha=0.3)
        ax.legend(loc="best", fontsize=7, ncol=2)
        ax.set_title(f"{name}: {ch['n_defined']} flights, {len(ch['magnitude_outliers'])} leave the fences, "
                     f"{'no outliergram' if ch['shape_outliers'] is None else str(len(ch['shape_outliers'])) + ' shape outliers'}",
                     fontsize=9)
    if len(names):
        axes[-1].set_xlabel("Row (node, fragment)" if "fragments" in result else "Time (s)")
    fig.tight_layout()
    return fig


def impact_point_figure(result):
    """The IIP trace from the dict of MonteCarloAnalyzer.impact_point_trace: the IIP range over the time of termination
    (the median - the quantile nearest 0.5 - and the outer and inner quantile bands), the ground track of the median IIP
    with the keep-in outline, and the exit times (one mark per quantile of statistics['exit_time'])."""
    q = np.asarray(result["q"], dtype=np.float64)
    t = np.asarray(result["time"], dtype=np.float64)
    fig = _figure((13, 5))
    ax_r, ax_xy = fig.subplots(1, 2)
    order = np.argsort(q)
    mid = int(np.argmin(np.abs(q - 0.5))) if len(q) else None
    rng = result["range"]
    quant = np.asarray(rng["quantiles"], dtype=np.float64)
    for depth, alpha in ((0, 0.2), (1, 0.35)):   # the outer pair, then the inner one
        if len(q) >= 2 * (depth + 1):
            lo, hi = order[depth], order[len(q) - 1 - depth]
            ax_r.fill_between(t, quant[lo], quant[hi], alpha=alpha, color="tab:red", linewidth=0,
                              label=f"{100 * q[lo]:g} - {100 * q[hi]:g} %")
    centre = (lambda ch: np.asarray(ch["quantiles"], dtype=np.float64)[mid]) if mid is not None else \
        (lambda ch: np.asarray(ch["mean"], dtype=np.float64))
    ax_r.plot(t, centre(rng), color="tab:red", linewidth=1.5, label=f"{100 * q[mid]:g} %" if mid is not None else "mean")
    exits = (result.get("statistics") or {}).get("exit_time")
    if exits and exits.get("count", 0) > 0:
        for v in exits["quantiles"]:
            if np.isfinite(v):
                ax_r.axvline(float(v), color="black", linewidth=0.8, linestyle="--")
    p = result.get("exit_probability", float("nan"))
    title = "IIP Range over Termination Time"
    if np.isfinite(p):
        lo, hi = result.get("exit_interval", (0.0, 1.0))
        title += f"\nP(IIP leaves keep-in) = {100 * p:.2f} % [{100 * lo:.2f}, {100 * hi:.2f}]"
    ax_r.set_title(title)
    ax_r.set_xlabel("Time of Termination since Rail Exit (s)")
    ax_r.set_ylabel("IIP Range (m)")
    ax_r.grid(True, alpha=0.3)
    ax_r.legend(loc="best", fontsize=8)
    ax_xy.plot(centre(result["x"]), centre(result["y"]), color="tab:red", linewidth=1.5, marker=".", markersize=3,
               label="median IIP" if mid is not None else "mean IIP")
    keep = result.get("keep_in")
    if keep:
        kx, ky = [v[0] for v in keep] + [keep[0][0]], [v[1] for v in keep] + [keep[0][1]]
        ax_xy.plot(kx, ky, color="black", linewidth=1.2, label="keep-in area")
    ax_xy.set_title(f"IIP Ground Track ({int(result.get('n_counted', 0))} samples)")
    ax_xy.set_xlabel("X (m)")
    ax_xy.set_ylabel("Y (m)")
    ax_xy.grid(True, alpha=0.3)
    ax_xy.legend(loc="best", fontsize=8)
    fig.tight_layout()
    return fig


def debris_footprint_figure(result, node=None):
    """The debris footprint from the dict of MonteCarloAnalyzer.debris_footprint: per fragment the median impact range (the
    quantile nearest 0.5) with its outermost quantile band over the time of break-up, and the footprint at `node` (default
    the last one) - per fragment the box of the outermost X and Y quantiles about the median impact, the count grid of
    result['maps'] where that (node, fragment) has one - with the keep-in outline."""
    q = np.asarray(result["q"], dtype=np.float64)
    t = np.asarray(result["time"], dtype=np.float64)
    frags = list(result["fragments"])
    node = len(t) - 1 if node is None else int(node)
    if not 0 <= node < len(t):
        raise ValueError(f"node must be 0 to {len(t) - 1}")
    fig = _figure((13, 5))
    ax_r, ax_xy = fig.subplots(1, 2)
    order = np.argsort(q)
    mid = int(np.argmin(np.abs(q - 0.5))) if len(q) else None
    lo, hi = (order[0], order[-1]) if len(q) >= 2 else (None, None)
    centre = (lambda ch: np.asarray(ch["quantiles"], dtype=np.float64)[mid]) if mid is not None else \
        (lambda ch: np.asarray(ch["mean"], dtype=np.float64))
    rng_q = np.asarray(result["range"]["quantiles"], dtype=np.float64)      # [n_q, nodes, F]
    colors = [f"C{f % 10}" for f in range(len(frags))]
    for f, (beta, dv) in enumerate(frags):
        label = f"beta {beta:g} kg/m2, dv {dv:g} m/s"
        if lo is not None:
            ax_r.fill_between(t, rng_q[lo][:, f], rng_q[hi][:, f], alpha=0.15, color=colors[f], linewidth=0)
        ax_r.plot(t, centre(result["range"])[:, f], color=colors[f], linewidth=1.4, label=label)
    p = result.get("exit_probability", float("nan"))
    title = "Debris Impact Range over Break-up Time"
    if lo is not None:
        title += f" (median, {100 * q[lo]:g} - {100 * q[hi]:g} %)"
    if np.isfinite(p):
        a, b = result.get("exit_interval", (0.0, 1.0))
        title += f"\nP(a fragment leaves keep-in) = {100 * p:.2f} % [{100 * a:.2f}, {100 * b:.2f}]"
    ax_r.set_title(title)
    ax_r.set_xlabel("Time of Break-up since Rail Exit (s)")
    ax_r.set_ylabel("Impact Range (m)")
    ax_r.grid(True, alpha=0.3)
    ax_r.legend(loc="best", fontsize=7)
    maps = result.get("maps") or {}
    for f in range(len(frags)):
        m = maps.get((node, f))
        if m is not None and np.asarray(m["counts"]).sum() > 0:
            counts = np.asarray(m["counts"], dtype=np.float64)
            ax_xy.pcolormesh(np.asarray(m["edges_x"]), np.asarray(m["edges_y"]), np.where(counts > 0, counts, np.nan).T,
                             cmap="Greys", alpha=0.6, shading="flat")
        cx, cy = centre(result["x"])[node, f], centre(result["y"])[node, f]
        if lo is not None:
            xq, yq = np.asarray(result["x"]["quantiles"], dtype=np.float64), np.asarray(result["y"]["quantiles"], dtype=np.float64)
            x0, x1, y0, y1 = xq[lo][node, f], xq[hi][node, f], yq[lo][node, f], yq[hi][node, f]
            if np.isfinite([x0, x1, y0, y1]).all():
                ax_xy.plot([x0, x1, x1, x0, x0], [y0, y0, y1, y1, y0], color=colors[f], linewidth=1.0)
        if np.isfinite(cx) and np.isfinite(cy):
            ax_xy.plot([cx], [cy], color=colors[f], marker="o", markersize=4, linestyle="none")
    keep = result.get("keep_in")
    if keep:
        kx, ky = [v[0] for v in keep] + [keep[0][0]], [v[1] for v in keep] + [keep[0][1]]
        ax_xy.plot(kx, ky, color="black", linewidth=1.2, label="keep-in area")
        ax_xy.legend(loc="best", fontsize=8)
    ax_xy.set_title(f"Footprint of a Break-up at {t[node]:g} s ({int(result.get('n_counted', 0))} samples)")
    ax_xy.set_xlabel("X (m)")
    ax_xy.set_ylabel("Y (m)")
    ax_xy.grid(True, alpha=0.3)
    fig.tight_layout()
    return fig


def casualty_figure(result):
    """The dict of analysis.casualty_expectation in three panels: the individual-risk map - the smoothed one, or the counted
    one where the call did not smooth - as an image with one contour per level of result['levels'] over the outlines of the
    population raster; Ec given a break-up at t over the time of break-up (the node index without times) with what every
    node adds to Ec, p_fail * Ec|t, on a second axis; one bar per fragment class with its contribution to Ec."""
    pop = result.get("population")
    pop = None if pop is None else np.asarray(pop.cpu() if hasattr(pop, "cpu") else pop, dtype=np.float64)
    smooth = result.get("risk_smooth") is not None
    risk = np.asarray(result["risk_smooth"] if smooth else result["risk_count"], dtype=np.float64)
    ex, ey = np.asarray(result["edges_x"]), np.asarray(result["edges_y"])
    cx, cy = np.asarray(result["centres_x"]), np.asarray(result["centres_y"])
    fig = _figure((16, 5))
    ax_m, ax_t, ax_f = fig.subplots(1, 3)
    mesh = ax_m.pcolormesh(ex, ey, np.ma.masked_less_equal(risk.T, 0.0), cmap="magma_r", shading="flat")
    fig.colorbar(mesh, ax=ax_m, label="individual risk per launch")
    if pop is not None and pop.shape == risk.shape and len(cx) > 1 and len(cy) > 1 and pop.max() > pop.min():
        ax_m.contour(cx, cy, pop.T, levels=[0.5 * (pop.min() + pop.max())], colors="tab:blue", linewidths=0.8, linestyles="dashed")
    levels = sorted(float(v) for v in result.get("levels", ()))
    drawn = [lv for lv in levels if len(cx) > 1 and len(cy) > 1 and risk.min() < lv < risk.max()]
    if drawn:
        cs = ax_m.contour(cx, cy, risk.T, levels=drawn, colors="black", linewidths=1.0)
        ax_m.clabel(cs, fmt=lambda v: f"{v:.0e}", fontsize=7)
    kind = "smoothed" if smooth else "counted"
    ax_m.set_title(f"Individual Risk ({kind}); Ec = {result['ec']:.3g} +- {result['ec_se']:.2g}\n"
                   f"missing jobs {100 * result['missing_share']:.1f} %, off the raster {result['off_grid']}")
    ax_m.set_xlabel("X (m)")
    ax_m.set_ylabel("Y (m)")
    node_ec = np.asarray(result["per_node"]["ec"], dtype=np.float64)
    t = result.get("time")
    t = np.arange(len(node_ec), dtype=np.float64) if t is None else np.asarray(t, dtype=np.float64)
    ax_t.plot(t, node_ec, color="tab:red", linewidth=1.4, label="Ec given break-up at t")
    ax_t.set_xlabel("Time of Break-up (s)" if result.get("time") is not None else "Node")
    ax_t.set_ylabel("Expected Casualties given Break-up")
    ax_t.grid(True, alpha=0.3)
    ax_c = ax_t.twinx()
    ax_c.bar(t, np.asarray(result["ec_contribution"], dtype=np.float64), width=0.6 * (t[1] - t[0] if len(t) > 1 else 1.0),
             color="tab:gray", alpha=0.4, label="contribution to Ec")
    ax_c.set_ylabel("p_fail * Ec given Break-up")
    ax_t.set_title("Ec over the Time of Break-up")
    ax_t.legend(loc="upper left", fontsize=8)
    frag_ec = np.asarray(result["per_fragment"]["ec"], dtype=np.float64)
    frags = list(result.get("fragments") or [None] * len(frag_ec))
    labels = [f"{f}" if fr is None else f"{fr[0]:g} x {fr[1]:g} m2, {fr[2]:g} kg" for f, fr in enumerate(frags)]
    ax_f.bar(np.arange(len(frag_ec)), frag_ec, color=[f"C{f % 10}" for f in range(len(frag_ec))])
    ax_f.set_xticks(np.arange(len(frag_ec)))
    ax_f.set_xticklabels(labels, rotation=30, ha="right", fontsize=7)
    ax_f.set_ylabel("Contribution to Ec")
    ax_f.set_title("Ec by Fragment Class")
    ax_f.grid(True, axis="y", alpha=0.3)
    fig.tight_layout()
    return fig


def sobol_figure(result):
    """The dict of analysis.sobol_indices as paired bars: per row one panel, per group the first-order index S1 and the
    total-effect index ST side by side in the order of `group_names`, their bootstrap percentile intervals (lo, hi) as
    whiskers where there are replicates.  A NaN index (a constant row, an empty population) draws no bar."""
    names = list(result["group_names"])
    rows = list(result["row_names"])
    k = len(names)
    fig = _figure((max(6.0, 0.9 * k + 2.0), 3.0 * len(rows) + 0.8))
    axes = np.atleast_1d(fig.subplots(len(rows), 1, sharex=True))
    x = np.arange(k, dtype=np.float64)
    for j, (ax, row) in enumerate(zip(axes, rows)):
        for which, label, shift, color in (("first", "S1 (first order)", -0.2, "tab:blue"),
                                           ("total", "ST (total effect)", 0.2, "tab:orange")):
            est = np.asarray(result[which]["estimate"], dtype=np.float64)[j]
            lo = np.asarray(result[which]["lo"], dtype=np.float64)[j]
            hi = np.asarray(result[which]["hi"], dtype=np.float64)[j]
            ax.bar(x + shift, np.nan_to_num(est, nan=0.0), width=0.4, color=color, label=label)
            have = np.isfinite(est) & np.isfinite(lo) & np.isfinite(hi)
            if have.any():
                # a percentile interval need not hold the estimate: the whisker never has a negative arm
                err = np.vstack([np.maximum(est - lo, 0.0), np.maximum(hi - est, 0.0)])[:, have]
                ax.errorbar((x + shift)[have], est[have], yerr=err, fmt="none", ecolor="black", capsize=3, linewidth=0.8)
        ax.axhline(0.0, color="black", linewidth=0.6)
        count = int(np.asarray(result["count"])[j])
        ax.set_ylabel(row)
        ax.set_title(f"{row}: {count} design rows, interaction {float(np.asarray(result['interaction'])[j]):.3f}", fontsize=9)
        ax.grid(True, axis="y", alpha=0.3)
    axes[0].legend(loc="best", fontsize=8)
    axes[-1].set_xticks(x)
    axes[-1].set_xticklabels(names, rotation=45, ha="right")
    fig.suptitle(f"Sobol indices ({int(result['n_base'])} x {k + 2} flights)")
    fig.tight_layout()
    return fig


def surrogate_figure(result, top=8):
    """The dict of analysis.polynomial_chaos: per row three panels - the first-order and total indices of the variables as
    paired bars in the order of `names`, the `top` largest pair indices as horizontal bars, and predicted against flown on
    the held-out members (result['validation'], where there is one) with the diagonal.  A NaN index draws no bar."""
    names = list(result["names"])
    rows = list(result["row_names"])
    V = len(names)
    fig = _figure((max(11.0, 0.45 * V + 8.0), 3.2 * len(rows) + 0.8))
    axes = np.atleast_2d(fig.subplots(len(rows), 3, gridspec_kw={"width_ratios": [2.2, 1.3, 1.0]}))
    x = np.arange(V, dtype=np.float64)
    val = result.get("validation")
    for j, row in enumerate(rows):
        ax = axes[j, 0]
        for which, label, shift, color in (("first", "first order", -0.2, "tab:blue"), ("total", "total", 0.2, "tab:orange")):
            ax.bar(x + shift, np.nan_to_num(np.asarray(result[which], dtype=np.float64)[j], nan=0.0), width=0.4, color=color, label=label)
        r2, q2 = float(np.asarray(result["r2"])[j]), float(np.asarray(result["q2"])[j])
        ax.set_title(f"{row}: r2 = {r2:.4f}, q2 = {q2:.4f} ({int(result['n_fit'])} fitted, {int(result['n_val'])} held out)", fontsize=9)
        ax.set_ylabel("share of the explained variance")
        ax.set_xticks(x)
        ax.set_xticklabels(names, rotation=45, ha="right", fontsize=7)
        ax.grid(True, axis="y", alpha=0.3)
        if j == 0:
            ax.legend(loc="best", fontsize=8)
        ax = axes[j, 1]
        pairs = list(result["interactions"][j])[:top]
        ax.barh(np.arange(len(pairs)), [p[2] for p in pairs], color="tab:green")
        ax.set_yticks(np.arange(len(pairs)))
        ax.set_yticklabels([f"{a} x {b}" for a, b, _ in pairs], fontsize=7)
        ax.invert_yaxis()
        ax.set_title("largest pair indices", fontsize=9)
        ax.grid(True, axis="x", alpha=0.3)
        ax = axes[j, 2]
        if val is not None and np.asarray(val["flown"]).shape[1] > 0:
            flown, pred = np.asarray(val["flown"], dtype=np.float64)[j], np.asarray(val["predicted"], dtype=np.float64)[j]
            ax.plot(flown, pred, ".", markersize=2, alpha=0.5)
            ends = [float(np.nanmin(flown)), float(np.nanmax(flown))]
            ax.plot(ends, ends, color="black", linewidth=0.8)
            ax.set_xlabel("flown")
            ax.set_ylabel("predicted")
            ax.set_title("held-out members", fontsize=9)
        else:
            ax.set_axis_off()
    fig.suptitle(f"Polynomial chaos surrogate: degree {int(result['degree'])}, order {int(result['order'])}, {int(result['n_terms'])} terms")
    fig.tight_layout()
    return fig


def given_data_figure(result, top=4):
    """The dict of analysis.given_data_sensitivity: per row two panels.  Left: delta of every factor as a bar, in the order
    of `factor_names`, with the null band - a tick at null_mean and a line up to null_hi - where there are shifts; a bar
    that does not clear its band is indistinguishable from no effect.  Right: the main-effect curves (the conditional mean
    of the row along the class centres, +- the conditional std as a band) of the `top` factors of the row's ranking, each
    against the factor's rank-scaled axis (class index / classes) so that factors of different units share it."""
    names = list(result["factor_names"])
    rows = list(result["row_names"])
    k = len(names)
    fig = _figure((max(9.0, 0.5 * k + 7.0), 3.2 * len(rows) + 0.8))
    axes = np.asarray(fig.subplots(len(rows), 2, squeeze=False))
    x = np.arange(k, dtype=np.float64)
    delta = result["delta"]
    for j, row in enumerate(rows):
        ax = axes[j, 0]
        est = np.asarray(delta["estimate"], dtype=np.float64)[j]
        mean = np.asarray(delta["null_mean"], dtype=np.float64)[j]
        hi = np.asarray(delta["null_hi"], dtype=np.float64)[j]
        ax.bar(x, np.nan_to_num(est, nan=0.0), width=0.6, color="tab:blue", label="delta")
        have = np.isfinite(mean) & np.isfinite(hi)
        if have.any():
            ax.errorbar(x[have], mean[have], yerr=np.vstack([np.zeros(int(have.sum())), np.maximum(hi[have] - mean[have], 0.0)]),
                        fmt="_", color="black", ecolor="black", capsize=3, linewidth=0.8,
                        label=f"null mean .. {100 * float(result['level']):g} %")
        ax.set_ylabel(row)
        ax.set_title(f"{row}: delta of {int(result['count'])} samples", fontsize=9)
        ax.set_xticks(x)
        ax.set_xticklabels(names if j == len(rows) - 1 else [""] * k, rotation=45, ha="right")
        ax.grid(True, axis="y", alpha=0.3)
        if j == 0:
            ax.legend(loc="best", fontsize=8)
        ax = axes[j, 1]
        for name in list(result["ranking"][j])[:top]:
            c = result["curves"][j][name]
            m, s = np.asarray(c["mean"], dtype=np.float64), np.asarray(c["std"], dtype=np.float64)
            u = (np.arange(len(m)) + 0.5) / max(len(m), 1)
            (line,) = ax.plot(u, m, marker="o", markersize=3, linewidth=1.2, label=name)
            ax.fill_between(u, m - s, m + s, alpha=0.12, color=line.get_color(), linewidth=0)
        ax.set_title(f"{row}: main effects", fontsize=9)
        ax.set_xlabel("factor quantile" if j == len(rows) - 1 else "")
        ax.grid(True, alpha=0.3)
        ax.legend(loc="best", fontsize=7)
    fig.suptitle(f"Given-data sensitivity ({int(result['classes'])} x {int(result['cells'])} classes, {int(result['shifts'])} shifts)")
    fig.tight_layout()
    return fig


def run_comparison_figure(cmp):
    """The dict of analysis.compare_runs (or TrajectoryEngine.compare): per row three panels - the two empirical
    distribution functions from the ECDF knots with the Kolmogorov-Smirnov location marked, the shift function (quantile of B
    minus quantile of A at the requested fractions), and the histogram of the null values of the Kolmogorov-Smirnov numerator
    with the observed one when the nulls were kept (otherwise the three p-values as text) - and a last row with the 1- and
    2-sigma ellipses of the two impact clouds, the energy statistic and its p-value.  No sample is needed."""
    rows = cmp["row"]
    R = len(rows)
    has_cloud = cmp.get("energy") is not None and cmp.get("cloud_a") is not None and cmp.get("cloud_b") is not None
    fig = _figure((13.0, 3.0 * (R + (1 if has_cloud else 0)) + 0.8))
    axes = np.asarray(fig.subplots(R + (1 if has_cloud else 0), 3, squeeze=False))
    levels = np.asarray(cmp["ecdf"]["levels"], dtype=np.float64)
    null = cmp.get("null_values")
    if null is not None and hasattr(null, "cpu"):
        null = null.cpu().numpy()
    q = np.asarray(cmp["q"], dtype=np.float64)
    for j, row in enumerate(rows):
        name = row.get("name", f"row {cmp['rows'][j]}")
        ax = axes[j, 0]
        if len(levels):
            ax.step(np.asarray(cmp["ecdf"]["a"])[j], levels, where="post", color="tab:blue", label=f"A ({cmp['count_a']})")
            ax.step(np.asarray(cmp["ecdf"]["b"])[j], levels, where="post", color="tab:orange", label=f"B ({cmp['count_b']})")
        if np.isfinite(row["ks_at"]):
            ax.axvline(row["ks_at"], color="black", linestyle=":", linewidth=0.9,
                       label=f"D = {row['ks']['statistic']:.4f} at {row['ks_at']:.6g}")
        ax.set_title(f"{name}: distribution functions", fontsize=9)
        ax.set_ylabel("F")
        ax.grid(True, alpha=0.3)
        ax.legend(loc="best", fontsize=7)
        ax = axes[j, 1]
        if len(q):
            ax.plot(q, np.asarray(row["shift"], dtype=np.float64), marker="o", color="tab:green")
        ax.axhline(0.0, color="black", linewidth=0.7)
        ax.set_title(f"{name}: shift function (B - A)", fontsize=9)
        ax.set_xlabel("quantile")
        ax.grid(True, alpha=0.3)
        ax = axes[j, 2]
        text = ", ".join(f"p({k}) = {row[k]['p_value']:.3g}" for k in ("ks", "mw", "cvm"))
        if null is not None and null.shape[1] > 0:
            ax.hist(null[3 * j], bins=min(40, max(5, null.shape[1] // 10)), color="0.7")
            ax.axvline(row["ks_num"], color="tab:red", label=f"observed K = {row['ks_num']}")
            ax.legend(loc="best", fontsize=7)
            ax.set_title(f"{name}: null of K; {text}", fontsize=8)
        else:
            ax.text(0.5, 0.5, row.get("verdict", text), ha="center", va="center", wrap=True, fontsize=8, transform=ax.transAxes)
            ax.set_title(f"{name}: {text}", fontsize=8)
            ax.set_xticks([])
            ax.set_yticks([])
    if has_cloud:
        ax = axes[R, 0]
        t = np.linspace(0.0, 2.0 * np.pi, 181)
        circle = np.vstack([np.cos(t), np.sin(t)])
        for key, color, label in (("cloud_a", "tab:blue", "A"), ("cloud_b", "tab:orange", "B")):
            c = cmp[key]
            mean, cov = np.asarray(c["mean"], dtype=np.float64), np.asarray(c["cov"], dtype=np.float64)
            w, v = np.linalg.eigh(cov)
            half = v @ np.diag(np.sqrt(np.maximum(w, 0.0)))
            for k in (1.0, 2.0):
                e = mean[:, None] + k * (half @ circle)
                ax.plot(e[0], e[1], color=color, linewidth=1.2 if k == 1.0 else 0.7, label=label if k == 1.0 else None)
            ax.plot(mean[0], mean[1], marker="+", color=color)
        e = cmp["energy"]
        ax.set_title(f"impact clouds (1, 2 sigma): E = {e['statistic']:.5g}, p = {e['p_value']:.3g}", fontsize=9)
        ax.set_xlabel("impact x")
        ax.set_ylabel("impact y")
        ax.grid(True, alpha=0.3)
        ax.legend(loc="best", fontsize=7)
        ax = axes[R, 1]
        ax.bar(["d_aa", "d_ab", "d_bb"], [e["d_aa"], e["d_ab"], e["d_bb"]], color=["tab:blue", "0.5", "tab:orange"])
        ax.set_title("mean distances", fontsize=9)
        ax.grid(True, axis="y", alpha=0.3)
        ax = axes[R, 2]
        if null is not None and null.shape[1] > 0:
            ax.hist(null[3 * R], bins=min(40, max(5, null.shape[1] // 10)), color="0.7")
            ax.axvline(e["statistic"], color="tab:red", label="observed E")
            ax.legend(loc="best", fontsize=7)
            ax.set_title("null of E", fontsize=9)
        else:
            ax.text(0.5, 0.5, cmp.get("energy_verdict", ""), ha="center", va="center", wrap=True, fontsize=8, transform=ax.transAxes)
            ax.set_xticks([])
            ax.set_yticks([])
    fig.suptitle(f"Run comparison ({int(cmp['permutations'])} permutations, level {float(cmp['level']):g})")
    fig.tight_layout()
    return fig


def exceedance_figure(tally, row="range", level=0.95):
    """The complementary distribution P(X > x) of one tallied row (the dict of analysis.tally_statistics /
    MonteCarloAnalyzer.run_monte_carlo_tally; row: its name) on a log axis: a step through the bin edges from the histogram
    counts (the mass above the range included), the held largest values as points at (value, rank / count) - the part of the
    tail the bins are too coarse for - and the Wilson score band at `level` around the steps.  A probability of zero has no
    place on a log axis: the curve ends at the last edge with mass above it."""
    from .analysis import wilson_interval
    r = tally["rows"][row]
    count = int(r["count"])
    fig = _figure((7.0, 4.5))
    ax = fig.subplots(1, 1)
    edges = np.asarray(r["histogram"]["edges"], dtype=np.float64)
    counts = np.asarray(r["histogram"]["counts"], dtype=np.int64)
    # counted values above edge i: the bins from i on and the mass above the range
    above = int(r["above"]) + np.concatenate([np.cumsum(counts[::-1])[::-1], [0]])
    have = above > 0
    if count > 0 and have.any():
        x, k = edges[have], above[have]
        band = np.array([wilson_interval(int(v), count, level) for v in k])
        ax.step(x, k / count, where="post", color="tab:blue", label="histogram")
        ax.fill_between(x, np.maximum(band[:, 0], 0.5 / count), band[:, 1], step="post", color="tab:blue", alpha=0.2,
                        label=f"{100 * level:.0f} % Wilson band")
    largest = r["largest"]
    if count > 0 and largest:
        # the e-th largest value is exceeded by e values (e = 0: by none, drawn at half a count)
        ax.plot([v for v, _ in largest], [max(e, 0.5) / count for e in range(len(largest))], "o", color="tab:red", markersize=3,
                label=f"{len(largest)} largest held")
    for t in r["exceedance"]:
        ax.axvline(t["threshold"], color="black", linewidth=0.6, linestyle="--")
    ax.set_yscale("log")
    ax.set_xlabel(row)
    ax.set_ylabel("P(X > x)")
    ax.set_title(f"{row}: exceedance over {count} counted flights")
    ax.grid(True, which="both", alpha=0.3)
    if count > 0:
        ax.legend(loc="best", fontsize=8)
    fig.tight_layout()
    return fig


def rare_event_figure(result, tally=None, row=None):
    """The exceedance curve P(g >= x) of a subset simulation (the dict of analysis.subset_simulation /
    MonteCarloAnalyzer.rare_event) on a log axis, down to its probability: the stitched curve, its log-normal band from the
    c.o.v. of the factors each point is conditioned on ('curve_cov'; at the result's interval_level), the level thresholds as
    dashed lines and the estimate itself with its interval at the target.  tally: optionally the dict of
    `run_monte_carlo_tally` whose row `row` (default: the result's) is drawn under it as the steps of `exceedance_figure` -
    direct Monte Carlo, where it still has counts.  A lower tail (g = -row) is drawn against g."""
    from scipy.special import ndtri
    curve = np.asarray(result["curve"], dtype=np.float64).reshape(-1, 2)
    cov = np.asarray(result.get("curve_cov", np.zeros(len(curve))), dtype=np.float64)
    z = float(ndtri(0.5 + 0.5 * float(result.get("interval_level", 0.95))))
    name = row or result.get("row", "g")
    fig = _figure((7.0, 4.5))
    ax = fig.subplots(1, 1)
    if tally is not None and name in tally.get("rows", {}):
        r = tally["rows"][name]
        count = int(r["count"])
        edges = np.asarray(r["histogram"]["edges"], dtype=np.float64)
        above = int(r["above"]) + np.concatenate([np.cumsum(np.asarray(r["histogram"]["counts"], dtype=np.int64)[::-1])[::-1], [0]])
        have = above > 0
        if count > 0 and have.any():
            ax.step(edges[have], above[have] / count, where="post", color="tab:gray", label=f"direct Monte Carlo, {count} flights")
    keep = curve[:, 1] > 0
    if keep.any():
        x, p = curve[keep, 0], curve[keep, 1]
        spread = np.exp(z * np.sqrt(np.log1p(cov[keep] ** 2)))
        ax.plot(x, p, color="tab:blue", label="subset simulation")
        ax.fill_between(x, p / spread, p * spread, color="tab:blue", alpha=0.2,
                        label=f"{100 * float(result.get('interval_level', 0.95)):.0f} % band")
    for lv in result.get("levels", []):
        ax.axvline(lv["threshold"], color="black", linewidth=0.6, linestyle="--")
    P = float(result["probability"])
    if result.get("target") is not None and P > 0:
        lo, hi = result["interval"]
        ax.errorbar([result["target"]], [P], yerr=[[P - lo], [hi - P]], fmt="o", color="tab:red", markersize=4, capsize=3,
                    label=f"P = {P:.3g} (c.o.v. {result['cov']:.2f})")
    ax.set_yscale("log")
    ax.set_xlabel(name if result.get("tail", "upper") == "upper" else f"-{name}")
    ax.set_ylabel("P(g >= x)")
    ax.set_title(f"{name}: {len(result.get('levels', []))} levels, {int(result.get('evaluations', 0))} evaluations")
    ax.grid(True, which="both", alpha=0.3)
    if ax.get_legend_handles_labels()[0]:
        ax.legend(loc="best", fontsize=8)
    fig.tight_layout()
    return fig


def save_figure(fig, output_dir, name):
    path = os.path.join(output_dir, name)
    fig.savefig(path, dpi=DPI, bbox_inches="tight")
    return path


# ---------------------------------------------------------------------------------------------- device layer
def device_inputs(analysis, device=None):
    """(engine, summary [16, n] float64, status [n] int32 or None) - device tensors of an analysis dict: the gathered tensors of
    `run_monte_carlo_device`, or ONE upload of the columns behind the LazyResults of `run_monte_carlo` (valid samples and
    outliers alike: the filter on the device finds the same split).  A plain list of result dicts (`_analyze_results`)
    is turned into columns first; rows it does not carry are NaN."""
    import torch
    from .simulator import shared_engine
    if "summary" in analysis and hasattr(analysis["summary"], "is_cuda"):
        summ, status = analysis["summary"], analysis.get("status")
        eng = shared_engine(summ.device if summ.is_cuda else device)
        summ = summ.to(device=eng.device, dtype=torch.float64).contiguous()
        if status is not None:
            status = status.to(device=eng.device, dtype=torch.int32).contiguous()
        return eng, summ, status
    eng = shared_engine(device)
    results = analysis["results"]
    table = getattr(results, "table", None)
    if table is not None:
        summ = torch.from_numpy(np.ascontiguousarray(table.summary, dtype=np.float64)).to(eng.device)
        status = torch.from_numpy(np.ascontiguousarray(table.status).astype(np.int32)).to(eng.device)
        return eng, summ, status
    records = list(results) + list(analysis.get("outliers", []))
    cols = np.full((_abi.SUMMARY_DIM, len(records)), np.nan)
    for i, r in enumerate(records):
        cols[_abi.SUM_APOGEE_ALT, i] = r.get("apogee_altitude", np.nan)
        cols[_abi.SUM_RANGE, i] = r.get("range", np.nan)
        cols[_abi.SUM_FLIGHT_TIME, i] = r.get("flight_time", np.nan)
        pos = r.get("impact_position")
        if pos is not None:
            cols[_abi.SUM_IMPACT_X:_abi.SUM_IMPACT_Z + 1, i] = pos
    return eng, torch.from_numpy(cols).to(eng.device), None


_REPORT_KEYS = ("n_samples", "n_failed", "n_outliers", "apogee_altitude", "range", "flight_time")


def _print_statistics(analysis):
    """monte_carlo.py:619-631."""
    print("\nMonte Carlo Analysis Results:")
    print(f"Number of valid simulations: {analysis['n_samples']}")
    print(f"Number of failed simulations: {analysis['n_failed']}")
    print(f"Number of outlier simulations: {analysis['n_outliers']}")
    for title, key in (("Apogee Altitude Statistics:", "apogee_altitude"), ("Range Statistics:", "range")):
        st = analysis[key]
        print(f"\n{title}")
        print(f"  Mean: {st['mean']:.1f} m")
        print(f"  Standard Deviation: {st['std']:.1f} m")
        print(f"  95% Confidence Interval: [{st['percentiles'][0]:.1f}, {st['percentiles'][4]:.1f}] m")


def plot_results(analyzer, analysis, save_plots=True):
    """MonteCarloAnalyzer.plot_results (monte_carlo.py:562-633)."""
    from . import analysis as analysis_mod
    eng, summ, status = device_inputs(analysis, analyzer.device)
    rows = [_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE, _abi.SUM_FLIGHT_TIME]
    dist = analysis_mod.native_distributions(summ, status, engine=eng, bins=50, rows=rows)
    points = density = None
    if dist["n_samples"] <= SCATTER_MAX:
        pair = summ[[_abi.SUM_APOGEE_ALT, _abi.SUM_RANGE]][:, dist["valid_mask"]].cpu().numpy()
        points = pair[:, np.isfinite(pair[0]) & np.isfinite(pair[1])]
    else:
        density = eng.histogram2d(summ, dist["outlier_reason_bits"], _abi.SUM_APOGEE_ALT, _abi.SUM_RANGE,
                                  bins=DENSITY_BINS)[:3]
    fig = distributions_figure([(dist[r]["edges"], dist[r]["counts"]) for r in rows], points=points, density=density)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Plots saved to: {save_figure(fig, output_dir, 'monte_carlo_distributions.png')}")
        if all(k in analysis for k in _REPORT_KEYS):
            analyzer._save_report(analysis, output_dir)
            print(f"Report saved to: {output_dir}")
    if all(k in analysis for k in _REPORT_KEYS):
        _print_statistics(analysis)
    return output_dir


def _trajectories_of(analysis, max_trajectories):
    return list(analysis.get("results", [])[:max_trajectories])


def plot_trajectory_cloud(analyzer, analysis, save_plots=True, max_trajectories=50):
    """MonteCarloAnalyzer.plot_trajectory_cloud (monte_carlo.py:635-677); returns the output directory."""
    fig = trajectory_cloud_figure(_trajectories_of(analysis, max_trajectories))
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Trajectory plots saved to: {save_figure(fig, output_dir, 'monte_carlo_trajectories.png')}")
    return output_dir


def plot_trajectory_cloud_3d(analyzer, analysis, save_plots=True, max_trajectories=50):
    """MonteCarloAnalyzer.plot_trajectory_cloud_3d (monte_carlo.py:679-707); returns the output directory."""
    fig = trajectory_cloud_3d_figure(_trajectories_of(analysis, max_trajectories))
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"3D trajectory plot saved to: {save_figure(fig, output_dir, 'monte_carlo_trajectories_3d.png')}")
    return output_dir


def plot_landing_dispersion(analyzer, analysis, save_plots=True, target=None):
    """Impact footprint, confidence ellipses and CEP of the filtered population (no reference counterpart): writes
    monte_carlo_landing.png and landing_dispersion.json (the dict of analysis.landing_dispersion); returns the output
    directory."""
    from .reports import to_serializable
    eng, summ, status = device_inputs(analysis, analyzer.device)
    res, why = eng.analyze(summ, status, rows=[], quantiles=[], reasons=True)
    disp = eng.dispersion(summ, why, centre=(0.0, 0.0) if target is None else target)
    disp["n_samples"], disp["n_outliers"] = int(res.n_valid), int(res.n_outliers)
    density = eng.histogram2d(summ, why, _abi.SUM_IMPACT_X, _abi.SUM_IMPACT_Y, bins=LANDING_BINS)[:3]
    fig = landing_figure(disp, density=density)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Landing dispersion plot saved to: {save_figure(fig, output_dir, 'monte_carlo_landing.png')}")
        with open(os.path.join(output_dir, "landing_dispersion.json"), "w") as fh:
            json.dump(to_serializable(disp), fh, indent=2)
    return output_dir


def plot_impact_probability(analyzer, analysis, save_plots=True, zones=None, **kw):
    """The impact probability map of the filtered population (no reference counterpart): writes
    monte_carlo_impact_probability.png and impact_probability.json (the dict of analysis.impact_probability without the
    per-sample row); returns the output directory (None without save_plots)."""
    from .reports import to_serializable
    res = analyzer.impact_probability(analysis, zones=zones, **kw)
    res.pop("sample_density", None)
    fig = impact_probability_figure(res)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Impact probability plot saved to: {save_figure(fig, output_dir, 'monte_carlo_impact_probability.png')}")
        with open(os.path.join(output_dir, "impact_probability.json"), "w") as fh:
            json.dump(to_serializable(res), fh, indent=2)
    return output_dir


def plot_reweighted_impact(analyzer, reweighted, save_plots=True):
    """The map of MonteCarloAnalyzer.reweighted_impact (no reference counterpart): writes monte_carlo_reweighted_impact.png
    and reweighted_impact.json (the dict without the per-sample row); returns the output directory (None without
    save_plots)."""
    from .reports import to_serializable
    res = {k: v for k, v in reweighted.items() if k != "sample_density"}
    fig = reweighted_impact_figure(res)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Reweighted impact plot saved to: {save_figure(fig, output_dir, 'monte_carlo_reweighted_impact.png')}")
        with open(os.path.join(output_dir, "reweighted_impact.json"), "w") as fh:
            json.dump(to_serializable(res), fh, indent=2)
    return output_dir


def plot_trajectory_corridor(analyzer, corridor, save_plots=True):
    """The corridor of MonteCarloAnalyzer.trajectory_corridor (no reference counterpart) as monte_carlo_corridor.png;
    returns the output directory (None without save_plots)."""
    fig = corridor_figure(corridor)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Trajectory corridor plot saved to: {save_figure(fig, output_dir, 'monte_carlo_corridor.png')}")
    return output_dir


def plot_reweighted_corridor(analyzer, reweighted, save_plots=True):
    """The corridor of MonteCarloAnalyzer.reweighted_corridor (no reference counterpart): writes
    monte_carlo_reweighted_corridor.png and reweighted_corridor.json next to it; returns the output directory (None without
    save_plots)."""
    from .reports import to_serializable
    fig = reweighted_corridor_figure(reweighted)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Reweighted corridor plot saved to: {save_figure(fig, output_dir, 'monte_carlo_reweighted_corridor.png')}")
        with open(os.path.join(output_dir, "reweighted_corridor.json"), "w") as fh:
            json.dump(to_serializable(reweighted), fh, indent=2)
    return output_dir


def plot_corridor_drivers(analyzer, drivers, save_plots=True, top=4):
    """The drivers of MonteCarloAnalyzer.corridor_drivers (no reference counterpart) as monte_carlo_corridor_drivers.png with
    save_plots; returns the figure."""
    fig = corridor_drivers_figure(drivers, top)
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Corridor drivers plot saved to: {save_figure(fig, output_dir, 'monte_carlo_corridor_drivers.png')}")
    return fig


def plot_functional_boxplot(analyzer, depth, values=None, save_plots=True, most=20):
    """The result of MonteCarloAnalyzer.trajectory_depth (no reference counterpart) as monte_carlo_functional_boxplot.png with
    save_plots; returns the figure."""
    fig = functional_boxplot_figure(depth, values, most)
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Functional boxplot saved to: {save_figure(fig, output_dir, 'monte_carlo_functional_boxplot.png')}")
    return fig


def plot_impact_point_trace(analyzer, trace, save_plots=True):
    """The IIP trace of MonteCarloAnalyzer.impact_point_trace (no reference counterpart) as monte_carlo_impact_points.png;
    returns the output directory (None without save_plots)."""
    fig = impact_point_figure(trace)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Impact point trace plot saved to: {save_figure(fig, output_dir, 'monte_carlo_impact_points.png')}")
    return output_dir


def plot_debris_footprint(analyzer, footprint, node=None, save_plots=True):
    """The footprint of MonteCarloAnalyzer.debris_footprint (no reference counterpart) as monte_carlo_debris.png; returns the
    output directory (None without save_plots)."""
    fig = debris_footprint_figure(footprint, node)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Debris footprint plot saved to: {save_figure(fig, output_dir, 'monte_carlo_debris.png')}")
    return output_dir


def plot_casualty(analyzer, casualty, save_plots=True):
    """The result of MonteCarloAnalyzer.casualty_expectation (no reference counterpart) as monte_carlo_casualty.png; returns the
    output directory (None without save_plots)."""
    fig = casualty_figure(casualty)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Casualty expectation plot saved to: {save_figure(fig, output_dir, 'monte_carlo_casualty.png')}")
    return output_dir


def plot_drivers(analyzer, analysis, save_plots=True):
    """One tornado chart per default row (apogee, range, flight time) of `MonteCarloAnalyzer.drivers(analysis)`, stacked
    in monte_carlo_drivers.png; returns the output directory (None without save_plots)."""
    import io

    from matplotlib import image as mpimg
    d = analyzer.drivers(analysis)
    panels = [drivers_figure(d, j) for j in range(len(d["row_names"]))]
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        # the panels have different heights (one bar pair per factor drawn): render each, stack the images
        images = []
        for f in panels:
            buf = io.BytesIO()
            f.savefig(buf, dpi=DPI // 2, format="png")
            buf.seek(0)
            images.append(mpimg.imread(buf))
        width = max(im.shape[1] for im in images)
        sheet = np.ones((sum(im.shape[0] for im in images), width, 4), dtype=images[0].dtype)
        at = 0
        for im in images:
            sheet[at:at + im.shape[0], :im.shape[1], :im.shape[2]] = im
            at += im.shape[0]
        path = os.path.join(output_dir, "monte_carlo_drivers.png")
        mpimg.imsave(path, sheet)
        print(f"Drivers plot saved to: {path}")
    return output_dir


def plot_sobol(analyzer, sobol, save_plots=True):
    """The indices of MonteCarloAnalyzer.sobol_indices (no reference counterpart) as monte_carlo_sobol.png; returns the
    output directory (None without save_plots)."""
    fig = sobol_figure(sobol)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Sobol indices plot saved to: {save_figure(fig, output_dir, 'monte_carlo_sobol.png')}")
    return output_dir


def plot_surrogate(analyzer, surrogate, save_plots=True):
    """The surrogate of MonteCarloAnalyzer.surrogate (no reference counterpart) as monte_carlo_surrogate.png; returns the
    output directory (None without save_plots)."""
    fig = surrogate_figure(surrogate)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Surrogate plot saved to: {save_figure(fig, output_dir, 'monte_carlo_surrogate.png')}")
    return output_dir


def plot_given_data_sensitivity(analyzer, sensitivity, save_plots=True, top=4):
    """The measures of MonteCarloAnalyzer.given_data_sensitivity (no reference counterpart) as monte_carlo_given_data.png;
    returns the output directory (None without save_plots)."""
    fig = given_data_figure(sensitivity, top)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Given-data sensitivity plot saved to: {save_figure(fig, output_dir, 'monte_carlo_given_data.png')}")
    return output_dir


def plot_run_comparison(analyzer, comparison, save_plots=True):
    """The tests of MonteCarloAnalyzer.compare_runs (no reference counterpart) as monte_carlo_run_comparison.png; returns the
    output directory (None without save_plots)."""
    fig = run_comparison_figure(comparison)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Run comparison plot saved to: {save_figure(fig, output_dir, 'monte_carlo_run_comparison.png')}")
    return output_dir


def plot_exceedance(analyzer, tally, row="range", save_plots=True, level=0.95):
    """The exceedance curve of a tallied row (no reference counterpart) as monte_carlo_exceedance_<row>.png; returns the output
    directory (None without save_plots)."""
    fig = exceedance_figure(tally, row, level)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        print(f"Exceedance plot saved to: {save_figure(fig, output_dir, f'monte_carlo_exceedance_{row}.png')}")
    return output_dir


def plot_rare_event(analyzer, result, save_plots=True, tally=None):
    """The exceedance curve of `MonteCarloAnalyzer.rare_event` (no reference counterpart) as monte_carlo_rare_event_<row>.png;
    returns the output directory (None without save_plots)."""
    fig = rare_event_figure(result, tally)
    output_dir = None
    if save_plots:
        output_dir = analyzer._create_output_directory()
        name = f"monte_carlo_rare_event_{result.get('row', 'g')}.png"
        print(f"Rare-event plot saved to: {save_figure(fig, output_dir, name)}")
    return output_dir
