"""Evaluator steps per second with the health metrics, with and without the timeline.

One measurement per process, as tools/health_cost.py: builds the shape's layout, runs one small
warm-up evaluation (kernel loading), then times whole ``evacx.evaluate(metrics=True)`` calls (host
clock; the call ends in a device-to-host copy) and prints one JSON line: steps, seconds and steps
per second of every repeat. ``--timeline`` adds ``timeline=True`` (``--track N`` persons with it).
``--root DIR`` measures another checkout of the repository (e.g. the parent commit, built; it has no
``--timeline``), so one session can alternate the variants.

Usage: python tools/timeline_cost.py [--timeline [--track 20]] [--root DIR]
                                     [--grid 64 --people 569 --robots 8 --envs 4096]
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--timeline", action="store_true")
    ap.add_argument("--track", type=int, default=0)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--people", type=int, default=569)
    ap.add_argument("--robots", type=int, default=8)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=1)
    ap.add_argument("--policy", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "dqn-marl_amd")]
    import torch
    from evacx.env import DeviceLayout
    from evacx.evaluate import evaluate
    from evacx.layout import build_tables, synthetic
    kw = dict(metrics=True)
    if args.timeline:
        kw.update(timeline=True, track=args.track or None)
    lay = DeviceLayout(build_tables(synthetic(args.grid, args.grid, args.robots)), args.people)
    evaluate(lay, 64, 1, args.policy, **kw)
    torch.cuda.synchronize()
    runs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        ev = evaluate(lay, args.envs, args.episodes, args.policy, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        runs.append(dict(steps=ev["steps"], seconds=round(dt, 4), steps_per_s=round(ev["steps"] / dt, 1)))
    out = dict(label=args.label, root=root, timeline=args.timeline, track=args.track, envs=args.envs, grid=args.grid,
               people=args.people, robots=args.robots, runs=runs, avg_health=ev.get("avg_health"),
               death_rate=ev["death_rate"])
    if args.timeline:
        cv = ev["curves"]
        out.update(curve_episodes=cv["episodes"], late_steps=int(cv["late"][3]), bad_health=cv["bad_health"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
