"""Strategy comparison over many envs: evacx.evaluate(metrics=True) per strategy, one table.

Builds the env of ``configs/dqn.yaml`` with ``--robots`` robots, runs ``--envs`` copies of it
for ``--episodes`` episodes each under every strategy that applies, and prints one row per
strategy -- average health, death rate, evacuation rate, average time, episodes -- in the
terms of ``EvacuationEnv.get_performance_metrics()``; the same rows go to ``--out``
(``strategy_comparison.csv``).

Strategies: ``static`` (every robot keeps action 4) and ``random`` always; ``--dqn PATH`` one
network shared by every robot; ``--per-robot PATH...`` one network per robot (the
``double_dqn_agent{1,2}.pth`` checkpoints); ``--qmix PATH...`` the QMIX agents
(``qmix_agent{1,2}.pth``; the mixer plays no part in acting). A checkpoint is the reference's
dict (its ``q_network``) or a bare state_dict, conv or MLP.

``--curves``, ``--track N`` and ``--plot`` add how the evacuation went over time
(``evaluate(timeline=True)``): per strategy ``curves_<strategy>.csv`` (one row per step: newly
evacuated and dead, episodes running, mean evacuated / dead / remaining, average health),
``tracked_<strategy>.npz`` (the first N persons of env 0, step by step) and
``evaluation_<strategy>.png`` (``utils.visualization.plot_evaluation``; needs matplotlib).

``--maps`` adds where it happened (``evaluate(maps=True)``): per strategy ``maps_<strategy>.npz``
(per grid cell the persons that arrived, stalled, left through an exit or died there and the
robots' positions, with occupancy, density and the stall ratio; summed over the layouts), one
printed line with the exits' shares and the worst stall cell, and with ``--plot``
``maps_<strategy>.png`` (``utils.visualization.plot_maps``).

The reference's "no robot" strategy is not offered: it parks the robot at (1000, 1000), and
the vector kernels' tables are padded by 6 cells only, so they must not be fed off-grid
positions.

Usage: python -m Louvre_Evacuation.runners.evaluate_vec --envs 4096 --episodes 2   (from dqn-marl_amd/)
"""
import argparse
import csv
import os
import sys

project_root = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if project_root not in sys.path:
    sys.path.insert(0, project_root)

import torch  # noqa: E402
import yaml  # noqa: E402

MAPS_KEYS = ["arrive", "stall", "evac", "died", "robot", "occupancy", "density", "stall_ratio", "steps", "episodes",
             "bad", "exit_use", "hotspots"]
CSV_COLUMNS = ["strategy", "avg_health", "death_rate", "evac_rate", "avg_time", "episodes"]
CURVE_COLUMNS = ["step", "time_s", "new_evacuated", "new_dead", "ended", "running", "evacuated_mean", "dead_mean",
                 "remaining_mean", "avg_health"]
STATIC_ACTION = 4


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0],
                                 epilog="No 'no robot' strategy: the reference moves the robot to (1000, 1000), and "
                                        "the vector kernels' tables are padded by 6 cells only.")
    ap.add_argument("--config", default=os.path.join(project_root, "configs", "dqn.yaml"))
    ap.add_argument("--robots", type=int, default=1, help="robots per env (1: EvacuationEnv; 2: EvacuationEnvMulti)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=1, help="episodes per env and strategy")
    ap.add_argument("--dqn", default=None, metavar="PATH", help="one checkpoint, shared by every robot")
    ap.add_argument("--per-robot", nargs="+", default=None, metavar="PATH", help="one checkpoint per robot")
    ap.add_argument("--qmix", nargs="+", default=None, metavar="PATH", help="one QMIX agent checkpoint per robot")
    ap.add_argument("--out", default=None, help="output directory (default: the config's save_path)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seed-base", type=int, default=1234, help="env e is seeded seed_base + e under every strategy")
    ap.add_argument("--curves", action="store_true",
                    help="write curves_<strategy>.csv: one row per step (evacuated, dead, remaining, avg health ...)")
    ap.add_argument("--track", type=int, default=0, metavar="N",
                    help="write tracked_<strategy>.npz: the first N persons of env 0, step by step")
    ap.add_argument("--maps", action="store_true",
                    help="write maps_<strategy>.npz: occupancy, stalls, exit use, deaths and robot positions per cell")
    ap.add_argument("--plot", action="store_true",
                    help="write evaluation_<strategy>.png, and with --maps maps_<strategy>.png (needs matplotlib)")
    return ap


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def build_spec(env_cfg, robots: int):
    """The config's env with ``robots`` robots: EvacuationEnv's for one, EvacuationEnvMulti's
    placement for two, the scaled placement beyond."""
    from evacx.layout import LayoutSpec, reference_multi, reference_scaled_multi
    ex = env_cfg.get("exit_location", [36, 15])
    L, W, exit_ = int(env_cfg["width"]), int(env_cfg["height"]), (int(ex[0]), int(ex[1]))
    if robots == 1:
        return LayoutSpec(L=L, W=W, exit=exit_)
    if robots == 2:
        return reference_multi(L=L, W=W, exit=exit_)
    import dataclasses
    return dataclasses.replace(reference_scaled_multi(L, W, robots), exit=exit_)


def load_learner(path, device, seed: int = 0):
    """An eval-only evacx.qnet.Learner from a checkpoint: conv or MLP by the dict's keys."""
    from evacx.qnet import Learner
    sd = torch.load(path, map_location="cpu", weights_only=True)
    sd = sd.get("q_network", sd)
    lr = Learner(kind="conv" if "conv1.weight" in sd else "mlp", device=device, precision="f32", seed=seed)
    for k, shape in lr.shapes.items():
        if k not in sd or tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"{path}: {k} is missing or not of shape {tuple(shape)}")
    lr.online.load_state_dict(sd)
    lr.weights_written()
    return lr


def strategies(args, R: int, device):
    """(name, policy, learner) of every strategy the arguments ask for."""
    out = [("static", STATIC_ACTION, None), ("random", "random", None)]
    if args.dqn:
        out.append(("dqn", "greedy", load_learner(args.dqn, device)))
    for name, paths in (("per_robot", args.per_robot), ("qmix", args.qmix)):
        if not paths:
            continue
        if len(paths) != R:
            raise ValueError(f"--{name.replace('_', '-')}: {len(paths)} checkpoints for {R} robots")
        out.append((name, "greedy", [load_learner(p, device) for p in paths]))
    return out


def table_row(name, ev) -> list:
    """One CSV row of an evaluate(metrics=True) result (None where no episode has the number)."""
    return [name, ev["avg_health"], ev["death_rate"], ev["evac_rate"], ev["total_time_mean"], ev["episodes"]]


def _fmt(v, spec):
    return "n/a" if v is None else format(v, spec)


def write_curves(path, curves):
    """One row per step up to the last one at which an episode ran; floats as repr, NaN empty."""
    run = curves["running"]
    n = max((int(i) + 1 for i in run.nonzero()[0]), default=0)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CURVE_COLUMNS)
        for s in range(n):
            row = []
            for k in CURVE_COLUMNS:
                v = curves[k][s].item()
                row.append("" if v != v else repr(v))
            w.writerow(row)
    return n


def write_outputs(args, out_dir, name, ev, spec):
    """The per-strategy files --curves / --track / --plot ask for."""
    import numpy as np
    cv = ev["curves"]
    if args.curves:
        path = os.path.join(out_dir, f"curves_{name}.csv")
        n = write_curves(path, cv)
        print(f"{name}: {n} steps written to {path}" +
              (f" ({int(cv['late'][3])} steps beyond the table)" if cv["late"][3] else ""))
    if args.track:
        path = os.path.join(out_dir, f"tracked_{name}.npz")
        np.savez(path, **cv["tracked"])
        print(f"{name}: {len(cv['tracked']['len'])} tracked persons written to {path}")
    if args.plot:
        try:
            import matplotlib  # noqa: F401
        except ImportError:
            print(f"{name}: --plot needs matplotlib, which is not installed; no figure written")
            return
        from Louvre_Evacuation.utils.visualization import plot_evaluation
        path = plot_evaluation(ev, os.path.join(out_dir, f"evaluation_{name}.png"), layout=spec,
                               title=f"{name}: {ev['episodes']} episodes")
        print(f"{name}: figure written to {path}")


def maps_arrays(maps) -> dict:
    """The arrays of maps_<strategy>.npz (MAPS_KEYS) from ``evaluate(maps=True)["maps"]``: the entry
    summed over the layouts; ``exit_use`` rows (x, y, count, share) and ``hotspots`` rows (x, y, stall)
    as float64 / int64 tables."""
    import numpy as np
    m = maps["sum"]
    out = {k: np.asarray(m[k]) for k in MAPS_KEYS[:10]}
    out["bad"] = np.asarray(maps["bad"])
    out["exit_use"] = np.asarray(m["exit_use"], np.float64).reshape(-1, 4)
    out["hotspots"] = np.asarray(m["hotspots"], np.int64).reshape(-1, 3)
    return out


def maps_line(name, maps) -> str:
    """One line: every exit cell's share of the evacuated, and the cell where most persons stalled."""
    m = maps["sum"]
    use = m["exit_use"]
    exits = ", ".join(f"({x},{y}) {share:.1%}" for x, y, _, share in use[:8]) or "nobody evacuated"
    if len(use) > 8:
        exits += f", {len(use) - 8} more cells"
    hot = m["hotspots"]
    top = f"({hot[0][0]},{hot[0][1]}) with {hot[0][2]} person-steps" if hot else "none"
    return f"{name}: exit use {exits}; top stall cell {top}"


def write_maps(args, out_dir, name, ev, spec):
    """The per-strategy files --maps asks for, and its line."""
    import numpy as np
    path = os.path.join(out_dir, f"maps_{name}.npz")
    np.savez(path, **maps_arrays(ev["maps"]))
    print(maps_line(name, ev["maps"]))
    print(f"{name}: maps written to {path}")
    if args.plot:
        try:
            import matplotlib  # noqa: F401
        except ImportError:
            print(f"{name}: --plot needs matplotlib, which is not installed; no map figure written")
            return
        from Louvre_Evacuation.utils.visualization import plot_maps
        path = plot_maps(ev["maps"], os.path.join(out_dir, f"maps_{name}.png"), layout=spec,
                         title=f"{name}: {ev['episodes']} episodes")
        print(f"{name}: map figure written to {path}")


def evaluate_vec(args):
    from evacx.env import DeviceLayout
    from evacx.evaluate import evaluate
    from evacx.layout import build_tables
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_vec needs an MI355X (HIP) device; no CPU fallback exists")
    if args.robots < 1 or args.envs < 1 or args.episodes < 1:
        raise ValueError("--robots, --envs and --episodes must be >= 1")
    with open(args.config, "r", encoding="utf-8") as f:
        config = yaml.safe_load(f)
    ec = config["env"]
    out_dir = args.out or os.path.join(project_root, config.get("save_path", "dqn_results"))
    os.makedirs(out_dir, exist_ok=True)
    spec = build_spec(ec, args.robots)
    device = torch.device("cuda", torch.cuda.current_device())
    lay = DeviceLayout(build_tables(spec), int(ec["num_people"]), device=device)
    print(f"env {spec.L}x{spec.W}, {lay.P} people, {lay.R} robots, exit {tuple(spec.exit)}; {args.envs} envs x "
          f"{args.episodes} episodes per strategy on {device}")
    if not 0 <= args.track <= lay.P:
        raise ValueError(f"--track must be 0..{lay.P}")
    timeline = bool(args.curves or args.track or args.plot)
    extra = dict(timeline=True, track=args.track or None) if timeline else {}
    if args.maps:
        extra["maps"] = True
    rows = []
    for name, policy, learner in strategies(args, lay.R, device):
        ev = evaluate(lay, args.envs, args.episodes, policy, learner=learner, seed_base=args.seed_base,
                      seed=args.seed, metrics=True, **extra)
        rows.append(table_row(name, ev))
        if timeline:
            write_outputs(args, out_dir, name, ev, spec)
        if args.maps:
            write_maps(args, out_dir, name, ev, spec)
    print(f"{'strategy':<10} {'avg health':>10} {'death rate':>10} {'evac rate':>10} {'avg time':>9} {'episodes':>9}")
    for name, health, death, evac, time, n in rows:
        print(f"{name:<10} {_fmt(health, '10.2f')} {_fmt(death, '10.2%')} {_fmt(evac, '10.2%')} "
              f"{_fmt(time, '8.1f')}s {n:9d}")
    path = os.path.join(out_dir, "strategy_comparison.csv")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for row in rows:
            w.writerow([row[0]] + ["" if v is None else repr(v) for v in row[1:]])
    print(f"table written to {path}")
    return rows


def main(argv=None):
    return evaluate_vec(parse_args(argv))


if __name__ == "__main__":
    main()
