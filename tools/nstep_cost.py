#!/usr/bin/env python3
"""What n-step returns cost per training step ("n-step returns").

Builds two trainers of one shape -- VecTrainer(n_step=1) and VecTrainer(n_step=N) -- ages both
to the stationary episode phase the way bench.py does (random-action env steps with staggered
resets), and times blocks of training steps alternating between the two in one process, so clock
and neighbour noise hit both alike (one child process per shape). With n_step > 1 the learn step
samples with a launch of its own (the push launch's draw leaves no slot indices) and adds the
evx_replay_nstep launch. The host clock runs around a block that ends in a device synchronise.
Prints one JSON line per shape: ms per step of each variant per block, the means, each variant's
block min-max and the difference.

  python3 tools/nstep_cost.py                     # cfg3 and cfg2, n_step 1 against 3
  python3 tools/nstep_cost.py --shapes cfg2 --n-step 5 --steps 200 --rounds 6
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


def build(lay, E, R, opts, age_steps, stagger):
    from evacx.trainer import VecTrainer
    tr = VecTrainer(lay, E, batch=E, replay_capacity=capacity_for(E, R), **opts)
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
    ap.add_argument("--n-step", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100, help="training steps per timed block")
    ap.add_argument("--rounds", type=int, default=6, help="blocks per variant and shape")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--age-steps", type=int, default=1300)
    ap.add_argument("--stagger", type=int, default=1200)
    ap.add_argument("--schedule", choices=["strict", "lagged"], default="strict")
    args = ap.parse_args()
    if args.n_step < 2:
        sys.exit("--n-step must be >= 2 (it is compared with 1)")
    if not torch.cuda.is_available():
        sys.exit("nstep_cost.py needs the GPU")
    shapes = args.shapes.split(",")
    if len(shapes) > 1:
        # one fresh process per shape (the streams and allocations of earlier trainers stay with
        # a process and slow later ones: tools/episode_cost.py)
        import subprocess
        for name in shapes:
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shapes", name,
                                  "--schedule", args.schedule] +
                                 [a for k, v in (("--n-step", args.n_step), ("--steps", args.steps),
                                                 ("--rounds", args.rounds), ("--warmup", args.warmup),
                                                 ("--age-steps", args.age_steps), ("--stagger", args.stagger))
                                  for a in (k, str(v))])
            if rc:
                sys.exit(rc)
        return
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables_device, synthetic
    name = shapes[0]
    grid, P, R, E = SHAPES[name]
    lay = DeviceLayout(build_tables_device([synthetic(grid, grid, R)])[0], P)
    variants = {"n1": 1, f"n{args.n_step}": args.n_step}
    names = list(variants)
    trs = {k: build(lay, E, R, dict(n_step=variants[k], lagged_learn=args.schedule == "lagged"), args.age_steps,
                    args.stagger) for k in names}
    for tr in trs.values():
        block(tr, args.warmup)
    ms = {k: [] for k in names}
    for r in range(args.rounds):  # alternate, and swap who goes first
        for k in names[r % 2:] + names[:r % 2]:
            ms[k].append(block(trs[k], args.steps))
    for tr in trs.values():
        tr.env.check_err()
        assert torch.isfinite(tr.last_loss).all()
    nlen = trs[names[1]].samp["nlen"].float()
    mean = {k: float(np.mean(v)) for k, v in ms.items()}
    out = dict(shape=name, grid=grid, people=P, robots=R, envs=E, batch=E, schedule=args.schedule, replay="uniform",
               n_step=args.n_step, steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
               ms_per_step={k: [round(x, 4) for x in v] for k, v in ms.items()},
               mean={k: round(v, 4) for k, v in mean.items()},
               min={k: round(min(v), 4) for k, v in ms.items()}, max={k: round(max(v), 4) for k, v in ms.items()},
               delta_ms=round(mean[names[1]] - mean["n1"], 4),
               per_round_delta_ms=[round(b - a, 4) for a, b in zip(ms["n1"], ms[names[1]])],
               last_batch_mean_len=round(float(nlen.mean()), 3),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
