#!/usr/bin/env python3
"""What VecTrainer(episode_stats=True) costs per training step ("Episode statistics").

Builds two trainers of one shape, episode statistics off and on, ages both to the stationary
episode phase the way bench.py does (random-action env steps with staggered resets), and times
blocks of training steps alternating between the two in one process, so clock and neighbour
noise hit both alike (one child process per shape). Prints one JSON line per shape: ms per step of each variant per block, the
means, and the spread.

  python3 tools/episode_cost.py                     # cfg3 and cfg2
  python3 tools/episode_cost.py --shapes cfg2 --steps 200 --rounds 5
  rocprofv3 --kernel-trace --stats -d OUT -- python3 tools/episode_cost.py --profile 50
      # stats-on trainer only, 50 steps and one summary: the episode kernels' own times
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dqn-marl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# bench.py's configurations: grid, people, robots, envs (batch = envs)
SHAPES = {"cfg3": (128, 2276, 16, 32768), "cfg2": (64, 569, 8, 4096)}


def capacity_for(E, R):  # bench.py's default ring
    c = 1
    while c < 16 * E * R:
        c <<= 1
    return c


def build(lay, E, R, stats, age_steps, stagger):
    from evacx.trainer import VecTrainer
    tr = VecTrainer(lay, E, batch=E, replay_capacity=capacity_for(E, R), episode_stats=stats)
    env = tr.env
    gid = torch.arange(E, device="cuda")
    acts = torch.empty(E * R, device="cuda", dtype=torch.int32)
    g = torch.Generator(device="cuda").manual_seed(4321)
    for w in range(age_steps):
        torch.randint(0, 5, (E * R,), device="cuda", dtype=torch.int32, generator=g, out=acts)
        env.step(acts, auto_reset=True)
        if 0 < stagger and w < stagger:
            env.reset(mask=(gid % stagger == w) & ~env.done.bool())
    torch.cuda.synchronize()
    return tr


def block(tr, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.step()
    tr.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,cfg2")
    ap.add_argument("--steps", type=int, default=100, help="training steps per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="off / on block pairs per shape")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--age-steps", type=int, default=1300)
    ap.add_argument("--stagger", type=int, default=1200)
    ap.add_argument("--profile", type=int, default=0, metavar="N",
                    help="N steps of the stats-on trainer and one summary only (run under the profiler)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("episode_cost.py needs the GPU")
    shapes = args.shapes.split(",")
    if len(shapes) > 1:
        # one fresh process per shape: the fourth trainer built in one process (cfg2 with statistics,
        # after the two cfg3 trainers and cfg2 without) measured 0.37 ms per step against 0.245 ms in
        # a process that built only the cfg2 pair (the streams and allocations of earlier trainers
        # stay with a process), which says nothing about the statistics
        import subprocess
        for name in shapes:
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shapes", name] +
                                 [a for k, v in (("--steps", args.steps), ("--rounds", args.rounds),
                                                 ("--warmup", args.warmup), ("--age-steps", args.age_steps),
                                                 ("--stagger", args.stagger), ("--profile", args.profile))
                                  for a in (k, str(v))])
            if rc:
                sys.exit(rc)
        return
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables_device, synthetic
    for name in shapes:
        grid, P, R, E = SHAPES[name]
        lay = DeviceLayout(build_tables_device([synthetic(grid, grid, R)])[0], P)
        if args.profile:
            tr = build(lay, E, R, True, args.age_steps, args.stagger)
            block(tr, args.profile)
            s = tr.episode_summary()
            print(json.dumps(dict(shape=name, envs=E, profile_steps=args.profile, episodes=s["episodes"],
                                  return_mean=s["return_mean"], length_mean=s["length_mean"])), flush=True)
            del tr
            continue
        trs = {k: build(lay, E, R, k == "on", args.age_steps, args.stagger) for k in ("off", "on")}
        for tr in trs.values():
            block(tr, args.warmup)
        ms = {"off": [], "on": []}
        for r in range(args.rounds):
            for k in (("off", "on") if r % 2 == 0 else ("on", "off")):  # alternate, and alternate who goes first
                ms[k].append(block(trs[k], args.steps))
        t0 = time.perf_counter()
        s = trs["on"].episode_summary()
        t_sum = (time.perf_counter() - t0) * 1e3
        trs["on"].env.check_err()
        out = dict(shape=name, grid=grid, people=P, robots=R, envs=E, steps_per_block=args.steps, rounds=args.rounds,
                   warmup=args.warmup, ms_per_step_off=[round(x, 4) for x in ms["off"]],
                   ms_per_step_on=[round(x, 4) for x in ms["on"]],
                   mean_off=round(float(np.mean(ms["off"])), 4), mean_on=round(float(np.mean(ms["on"])), 4),
                   spread_off=round(max(ms["off"]) - min(ms["off"]), 4),
                   spread_on=round(max(ms["on"]) - min(ms["on"]), 4),
                   delta_ms=round(float(np.mean(ms["on"]) - np.mean(ms["off"])), 4),
                   summary_call_ms=round(t_sum, 3), episodes=s["episodes"], return_mean=s["return_mean"],
                   length_mean=s["length_mean"], evac_rate=s["evac_rate"], death_rate=s["death_rate"],
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(out), flush=True)
        del trs


if __name__ == "__main__":
    main()
