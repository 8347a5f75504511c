#!/usr/bin/env python3
"""What a population of K learners costs per training step against what a user does without it
(DESIGN.md 5.5).

One shape, three ways to spend a training step on K x E envs:
  (a) population  PopulationTrainer(K * E envs, members=K, batch B per member): grouped launches
  (b) separate    K VecTrainer(E envs, batch B, act_table=False), stepped one after another; their
                  block times are added -- K runs one after another in one process
  (c) one         one VecTrainer(K * E envs, batch B): one shared net, the floor of the same env work
All are aged to the stationary episode phase the way bench.py does (random-action env steps with
staggered resets) and timed in blocks of training steps alternating between the three in one process,
so clock and neighbour noise hit all alike; the host clock runs around a block that ends in a device
synchronise. Every shape runs in a child process of its own under a time limit. Prints one JSON line
per shape: ms per step of each variant per block, the means, the block min-max, (a) / (b).

  python3 tools/population_cost.py                      # cfg2: 8 x 4096 envs, B = 4096
  python3 tools/population_cost.py --members 4 --steps 200 --rounds 6
  python3 tools/population_cost.py --variants options   # the learner options' price list
  python3 tools/population_cost.py --variants population  # (a) alone: one build or commit against another
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dqn-marl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# grid, people, robots, envs per member (batch per member = envs per member)
SHAPES = {"cfg2": (64, 569, 8, 4096)}
LRS = (1e-3, 3e-4, 1e-4, 3e-5)
GAMMAS = (0.99, 0.95)


def capacity_for(E, R):  # bench.py's default ring
    c = 1
    while c < 16 * E * R:
        c <<= 1
    return c


def age(tr, E, R, age_steps, stagger):
    import torch
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


def block(trs, n):
    """ms per step of n steps of every trainer of trs, one trainer after another, added."""
    import torch
    total = 0.0
    for tr in trs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step()
        tr.sync()
        torch.cuda.synchronize()
        total += (time.perf_counter() - t0) * 1e3 / n
    return total


def child(args, name):
    import numpy as np
    import torch
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables_device, synthetic
    from evacx.population import PopulationTrainer
    from evacx.trainer import VecTrainer
    grid, P, R, E = SHAPES[name]
    K = args.members
    lay = DeviceLayout(build_tables_device([synthetic(grid, grid, R)])[0], P)
    cap = capacity_for(E, R)
    lrs = [LRS[k % len(LRS)] for k in range(K)]
    gammas = [GAMMAS[(k // len(LRS)) % len(GAMMAS)] for k in range(K)]
    def pop(**opts):
        return [age(PopulationTrainer(lay, K * E, members=K, batch=E, replay_capacity=cap, lr=lrs, gamma=gammas, **opts),
                    K * E, R, args.age_steps, args.stagger)]
    if args.variants == "options":  # the price list of the learner options: four populations of one shape
        soft = dict(double_q=True, loss="huber", huber_delta=1.0, target_tau=0.005)
        trs = {"population": pop(), "double_q": pop(double_q=True), "double_q_huber_tau": pop(**soft),
               "double_q_huber_tau_nstep3": pop(n_step=3, **soft)}
    elif args.variants == "population":  # variant (a) alone (two builds or two commits against each other)
        trs = {"population": pop()}
    else:
        trs = {
            "population": pop(),
            "separate": [age(VecTrainer(lay, E, batch=E, replay_capacity=cap, act_table=False, lr=lrs[k],
                                        gamma=gammas[k], learner_seed=k, seed_base=1234 + k * E), E, R, args.age_steps,
                             args.stagger) for k in range(K)],
            "one": [age(VecTrainer(lay, K * E, batch=E, replay_capacity=capacity_for(K * E, R)), K * E, R,
                        args.age_steps, args.stagger)],
        }
    names = list(trs)
    for k in names:
        block(trs[k], args.warmup)
    ms = {k: [] for k in names}
    for r in range(args.rounds):  # alternate, and rotate who goes first
        o = r % len(names)
        for k in names[o:] + names[:o]:
            ms[k].append(block(trs[k], args.steps))
    for group in trs.values():
        for tr in group:
            tr.env.check_err()
            assert torch.isfinite(tr.last_loss).all()
    mean = {k: float(np.mean(v)) for k, v in ms.items()}
    out = dict(shape=name, grid=grid, people=P, robots=R, members=K, envs_per_member=E, batch_per_member=E,
               steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
               ms_per_step={k: [round(x, 4) for x in v] for k, v in ms.items()},
               mean={k: round(v, 4) for k, v in mean.items()},
               min={k: round(min(v), 4) for k, v in ms.items()}, max={k: round(max(v), 4) for k, v in ms.items()},
               env_steps_per_s={k: round(K * E / (mean[k] * 1e-3)) for k in names},
               variants=args.variants, device=torch.cuda.get_device_name(0))
    if "separate" in mean:
        out["population_over_separate"] = round(mean["population"] / mean["separate"], 4)
    if args.variants == "options":  # per round: what each option set adds to the population's step
        out["over_population_ms"] = {k: [round(x - y, 4) for x, y in zip(ms[k], ms["population"])]
                                     for k in names if k != "population"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg2")
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100, help="training steps per timed block")
    ap.add_argument("--rounds", type=int, default=6, help="blocks per variant and shape")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--age-steps", type=int, default=1300)
    ap.add_argument("--stagger", type=int, default=1200)
    ap.add_argument("--limit", type=float, default=600.0, help="seconds a shape's child process may take")
    ap.add_argument("--variants", choices=["base", "options", "population"], default="base",
                    help="base: (a) / (b) / (c) above; options: the population with its learner options off, with "
                         "double_q, + Huber + target_tau 0.005 on every member, + n_step 3; population: (a) alone")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("population_cost.py needs the GPU")
        return child(args, args.child)
    for name in args.shapes.split(","):
        if name not in SHAPES:
            sys.exit(f"unknown shape {name!r} (one of {', '.join(SHAPES)})")
        # one fresh process per shape, under its own time limit; a shape that fails or runs out of
        # time ends the tool: nothing more is started on the device
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name] + \
              [a for k, v in (("--members", args.members), ("--steps", args.steps), ("--rounds", args.rounds),
                              ("--warmup", args.warmup), ("--age-steps", args.age_steps), ("--stagger", args.stagger),
                              ("--variants", args.variants))
               for a in (k, str(v))]
        try:
            rc = subprocess.call(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.limit:g} s")
        if rc:
            sys.exit(rc)


if __name__ == "__main__":
    main()
