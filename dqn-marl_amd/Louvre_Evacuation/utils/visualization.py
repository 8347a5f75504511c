"""Host-side performance log (counterpart of the reference utils/visualization.py:17-57)."""
from __future__ import annotations


class PerformanceRecorder:
    def __init__(self):
        self.episode_data = []
        self.step_data = []

    def record_episode(self, env, episode, total_reward):
        m = env.get_performance_metrics()
        self.episode_data.append({"episode": episode, "total_reward": total_reward, "evacuated": m["evacuated"],
                                  "dead": m["dead"], "remaining": m["remaining"],
                                  "evacuation_rate": m["evacuation_rate"], "death_rate": m["death_rate"],
                                  "avg_health": m["avg_health"], "min_health": m["min_health"],
                                  "total_steps": m["total_steps"]})

    def record_step(self, env, step, action, reward):
        m = env.get_performance_metrics()
        self.step_data.append({"step": step, "action": action, "reward": reward, "evacuated": m["evacuated"],
                               "dead": m["dead"], "remaining": m["remaining"], "avg_health": m["avg_health"]})

    def get_dataframe(self):
        import pandas as pd
        return pd.DataFrame(self.episode_data)


def visualize_trajectories(env, save_path=None):
    """Robot trajectory + final people positions (matplotlib, non-interactive)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(figsize=(6, 5))
    rt = [p for p, _ in env.robot_trajectory]
    if rt:
        ax.plot([p[0] for p in rt], [p[1] for p in rt], "b-", lw=1)
    ppl = env.people.list
    ax.scatter([p.pos[0] for p in ppl], [p.pos[1] for p in ppl], s=4,
               c=["g" if p.savety else ("k" if p.dead else "r") for p in ppl])
    ax.set_xlim(0, env.width + 2)
    ax.set_ylim(0, env.height + 2)
    if save_path:
        fig.savefig(save_path, dpi=100)
    plt.close(fig)


def _spans(curves):
    """Slots worth drawing: up to the last step at which an episode was still running."""
    import numpy as np
    run = np.asarray(curves["running"])
    on = np.nonzero(run > 0)[0]
    return slice(0, int(on[-1]) + 1 if len(on) else len(run))


def plot_evaluation(result, save_path, layout=None, title=None):
    """Four panels of one vector evaluation (``evacx.evaluate(..., timeline=True)``'s result, or its
    ``curves``), written to ``save_path`` as a PNG: where the tracked persons walked, over the
    layout when ``layout`` (a LayoutSpec / DeviceLayout: ``L``, ``W``, ``exit``) is given; their
    health next to the mean over every episode; when people got out and when they died; and how
    many were out, dead and still inside on average after each step."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import numpy as np
    cv = result.get("curves", result)
    sl = _spans(cv)
    t = np.asarray(cv["time_s"])[sl]
    trk = cv.get("tracked")
    fig, axes = plt.subplots(2, 2, figsize=(12, 9))
    (ax_map, ax_health), (ax_hist, ax_prog) = axes

    # who went where
    spec = getattr(layout, "spec", layout)
    if spec is not None:
        L, W = int(spec.L), int(spec.W)
        ax_map.plot([0.5, L + 0.5, L + 0.5, 0.5, 0.5], [0.5, 0.5, W + 0.5, W + 0.5, 0.5], color="0.4", lw=1)
        ax_map.plot([spec.exit[0]], [spec.exit[1]], marker="s", color="tab:green", ms=9, ls="", label="exit")
    if trk is not None and len(trk["len"]):
        for i, n in enumerate(np.asarray(trk["len"])):
            if n < 1:
                continue
            # an evacuated person's later slots repeat its last cell: draw up to the first safe slot
            ev = int(trk["evac_step"][i])
            end = int(n) if ev < 0 else min(int(n), ev + 1)
            xs, ys = trk["x"][:end, i], trk["y"][:end, i]
            fate = "tab:green" if ev >= 0 else ("black" if trk["death_step"][i] >= 0 else "tab:orange")
            ax_map.plot(xs, ys, lw=0.8, color=fate, alpha=0.7)
            ax_map.plot(xs[:1], ys[:1], marker=".", color=fate, ms=4)
    else:
        ax_map.text(0.5, 0.5, "no persons tracked", ha="center", va="center", transform=ax_map.transAxes)
    ax_map.set_aspect("equal", adjustable="datalim")
    ax_map.set_title("tracked persons (green: out, black: dead, orange: inside)")
    ax_map.set_xlabel("x")
    ax_map.set_ylabel("y")

    # health
    if trk is not None:
        for i, n in enumerate(np.asarray(trk["len"])):
            n = int(n)
            if n > 0:
                ax_health.plot(np.arange(n) * 0.5, trk["health"][:n, i], lw=0.6, color="tab:blue", alpha=0.4)
    ax_health.plot(t, np.asarray(cv["avg_health"])[sl], color="tab:red", lw=2,
                   label=f"mean of the not-dead, {cv['episodes']} episodes")
    ax_health.set_ylim(-2, 102)
    ax_health.set_xlabel("time [s]")
    ax_health.set_ylabel("health")
    ax_health.set_title("health")
    ax_health.legend(loc="lower left", fontsize=8)

    # the two distributions: persons per step of leaving / dying, per episode
    n_ep = max(int(cv["episodes"]), 1)
    ax_hist.bar(t, np.asarray(cv["new_evacuated"])[sl] / n_ep, width=0.5, color="tab:green", alpha=0.6,
                label="evacuated")
    ax_hist.bar(t, -np.asarray(cv["new_dead"])[sl] / n_ep, width=0.5, color="black", alpha=0.6, label="died (down)")
    ax_hist.axhline(0, color="0.3", lw=0.5)
    ax_hist.set_xlabel("time [s]")
    ax_hist.set_ylabel("persons per step and episode")
    ax_hist.set_title("evacuation times and death times")
    ax_hist.legend(fontsize=8)

    # progress
    for key, colour, name in (("evacuated_mean", "tab:green", "evacuated"), ("dead_mean", "black", "dead"),
                              ("remaining_mean", "tab:orange", "remaining")):
        ax_prog.plot(t, np.asarray(cv[key])[sl], color=colour, label=name)
    ax_run = ax_prog.twinx()
    ax_run.plot(t, np.asarray(cv["running"])[sl], color="0.6", ls=":", label="episodes running")
    ax_run.set_ylabel("episodes running")
    ax_prog.set_xlabel("time [s]")
    ax_prog.set_ylabel("persons (mean over episodes)")
    ax_prog.set_title("progress")
    ax_prog.legend(loc="center right", fontsize=8)
    if title:
        fig.suptitle(title)
    fig.tight_layout()
    fig.savefig(save_path, dpi=100, format="png")
    plt.close(fig)
    return save_path


def plot_maps(result, save_path, layout=None, title=None, row="sum"):
    """Four heat maps of one vector evaluation (``evacx.evaluate(..., maps=True)``'s result, or its
    ``maps``), written to ``save_path`` as a PNG: mean persons per cell and step (density), the
    share of them that stood still (stall ratio), where people died, and where the robots were;
    the exit cells carry their share of the evacuated. ``row`` picks a layout's entry instead of
    the sum; ``layout`` (``exit``) marks the configured exit."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import numpy as np
    m = result.get("maps", result)[row]
    spec = getattr(layout, "spec", layout)
    panels = (("density", "persons per cell and step", "viridis"), ("stall_ratio", "stall ratio", "magma"),
              ("died", "deaths", "Reds"), ("robot", "robot steps", "Blues"))
    fig, axes = plt.subplots(2, 2, figsize=(12, 9))
    for ax, (key, name, cmap) in zip(axes.reshape(-1), panels):
        a = np.asarray(m[key], np.float64).T  # [y][x]: x to the right, y upwards
        im = ax.imshow(a, origin="lower", cmap=cmap, interpolation="nearest")
        fig.colorbar(im, ax=ax, shrink=0.8)
        if spec is not None:
            ax.plot([spec.exit[0]], [spec.exit[1]], marker="s", mfc="none", color="tab:green", ms=9, ls="")
        ax.set_title(name)
        ax.set_xlabel("x")
        ax.set_ylabel("y")
    for x, y, _, share in m["exit_use"]:
        axes[0, 0].annotate(f"{share:.0%}", (x, y), color="white", fontsize=7, ha="center", va="center")
    if title:
        fig.suptitle(f"{title} ({m['steps']} env-steps)")
    fig.tight_layout()
    fig.savefig(save_path, dpi=100, format="png")
    plt.close(fig)
    return save_path
