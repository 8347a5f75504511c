"""What the spatial maps cost per evaluator step ("Spatial maps").

One process per shape. Builds the shape's synthetic layout and E envs, ages them, then times the
evaluator's step in three forms that take turns step by step over the same envs (``--repeats`` x
``--block`` steps of each), so each form sees the same mix of episode phases:

  fused    env.step(auto_reset=True) + EpisodeStats.update: evaluate(maps=False), the yardstick
  apart    env.step(auto_reset=False) + EpisodeStats.update + env.reset(mask=done): what
           metrics=True / timeline=True already run
  maps     apart + SpatialMaps.update before the reset and SpatialMaps.sync after it:
           evaluate(maps=True)

Every step is timed with device events around it, read after the loop (no host sync inside). Prints
one JSON line: the mean ms per step of every form (and per third of the run), the differences, the
update and sync launches alone, the plan's route and the traffic bound (8 B read and, for a person
whose pk changed, 4 B written per person and step).

Usage: python tools/spatial_cost.py [--grid 128 --people 2276 --robots 16 --envs 32768]
       python tools/spatial_cost.py --grid 256 --people 9102 --robots 1 --envs 8192
"""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--people", type=int, default=2276)
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--policy", type=int, default=4)
    ap.add_argument("--age", type=int, default=60, help="untimed fused steps before the first timed one")
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "dqn-marl_amd")]
    import torch
    from evacx.env import DeviceLayout, VecEnv
    from evacx.episodes import EpisodeStats
    from evacx.layout import build_tables, synthetic
    from evacx.spatial import SpatialMaps
    E = args.envs
    lay = DeviceLayout(build_tables(synthetic(args.grid, args.grid, args.robots)), args.people)
    env = VecEnv(lay, E)
    env.seed([1234 + i for i in range(E)])
    env.reset()
    stats = EpisodeStats(E, lay.device, lay.P)
    sm = SpatialMaps(E, lay.device, lay)
    sm.sync(env)
    actions = torch.full((E * lay.R,), args.policy, dtype=torch.int32, device=lay.device)

    def fused():
        env.step(actions, auto_reset=True)
        stats.update(env.reward, env.done, env.counts)

    def apart():
        env.step(actions, auto_reset=False)
        stats.update(env.reward, env.done, env.counts)
        env.reset(mask=env.done)

    def maps():
        env.step(actions, auto_reset=False)
        sm.update(env, env.done)
        stats.update(env.reward, env.done, env.counts)
        env.reset(mask=env.done)
        sm.sync(env, mask=env.done)

    forms = dict(fused=fused, apart=apart, maps=maps)
    for _ in range(args.age):
        fused()
    for f in forms.values():  # kernel loading
        f()
    torch.cuda.synchronize()

    def event():
        return torch.cuda.Event(enable_timing=True)
    # the three forms take turns step by step, so each sees the same mix of episode phases; every
    # step between its own two events, read after the loop
    marks = {k: [] for k in forms}
    parts = []  # the maps form's two calls alone
    for i in range(args.repeats * args.block):
        for name, f in forms.items():
            if name == "maps":
                sm.sync(env)  # the other forms moved the envs on: untimed
            t0, t1 = event(), event()
            t0.record()
            if name == "maps":
                u0, u1, s0, s1 = event(), event(), event(), event()
                env.step(actions, auto_reset=False)
                u0.record()
                sm.update(env, env.done)
                u1.record()
                stats.update(env.reward, env.done, env.counts)
                env.reset(mask=env.done)
                s0.record()
                sm.sync(env, mask=env.done)
                s1.record()
                parts.append((u0, u1, s0, s1))
            else:
                f()
            t1.record()
            marks[name].append((t0, t1))
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in marks.items()}
    update_ms = [u0.elapsed_time(u1) for u0, u1, _, _ in parts]
    sync_ms = [s0.elapsed_time(s1) for _, _, s0, s1 in parts]
    env.check_err()
    mean = {k: statistics.fmean(v) for k, v in ms.items()}
    m = sm.maps()
    persons = E * lay.P
    n = len(update_ms)
    thirds = {k: [round(statistics.fmean(v[j * n // 3:(j + 1) * n // 3]), 4) for j in range(3)] for k, v in ms.items()}
    out = dict(label=args.label, grid=args.grid, people=lay.P, robots=lay.R, envs=E, steps_per_form=n, age=args.age,
               plan=sm.plan(), ms_per_step={k: round(v, 4) for k, v in mean.items()}, ms_per_step_by_third=thirds,
               maps_minus_fused_ms=round(mean["maps"] - mean["fused"], 4),
               maps_minus_apart_ms=round(mean["maps"] - mean["apart"], 4),
               update_ms=round(statistics.fmean(update_ms), 4), update_ms_min_max=[round(min(update_ms), 4),
                                                                                   round(max(update_ms), 4)],
               sync_ms=round(statistics.fmean(sync_ms), 4),
               read_bytes_per_step=8 * persons, write_bytes_per_step_at_most=4 * persons,
               map_steps=m["sum"]["steps"], occupancy_sum=int(m["sum"]["occupancy"].sum()),
               stall_share=float(m["sum"]["stall"].sum() / max(int(m["sum"]["occupancy"].sum()), 1)), bad=m["bad"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
