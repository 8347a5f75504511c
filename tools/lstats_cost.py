#!/usr/bin/env python3
"""What the learner diagnostics cost per training step.

Builds three trainers of one shape -- the diagnostics off, VecTrainer(learn_stats=True), and
VecTrainer(learn_stats=True, value_probe=True) -- ages all three to the stationary episode phase
the way bench.py does (random-action env steps with staggered resets), and times blocks of training
steps alternating between them in one process, so clock and neighbour noise hit all alike (one
child process per shape). learn_stats adds two launches after clip + Adam; value_probe makes the
act write its Q rows and adds one launch per step beside the env step. The host clock runs around
a block that ends in a device synchronise. Prints one JSON line per shape: ms per step of each
variant per block, the means, each variant's block min-max and the differences per round.

  python3 tools/lstats_cost.py                     # cfg3 and cfg2, strict schedule
  python3 tools/lstats_cost.py --shapes cfg2 --schedule lagged --steps 200 --rounds 6
  python3 tools/lstats_cost.py --shapes cfg3 --schedule lagged --variants off,both,stats

--variants names the trainers to build and their order. In the lagged schedule the trainer built second
has measured slower than the first and third whatever its variant (its streams share hardware queues),
so compare trainers of like places, or build the variants in another order as well.
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
VARIANTS = {"off": dict(), "stats": dict(learn_stats=True), "both": dict(learn_stats=True, value_probe=True)}


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
    ap.add_argument("--steps", type=int, default=100, help="training steps per timed block")
    ap.add_argument("--rounds", type=int, default=6, help="blocks per variant and shape")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--age-steps", type=int, default=1300)
    ap.add_argument("--stagger", type=int, default=1200)
    ap.add_argument("--schedule", choices=["strict", "lagged"], default="strict")
    ap.add_argument("--variants", default="off,stats,both",
                    help="the trainers to build, in this order (off must be among them): a trainer's place in the "
                         "process decides which hardware queues its streams share")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstats_cost.py needs the GPU")
    shapes = args.shapes.split(",")
    if len(shapes) > 1:
        # one fresh process per shape (the streams and allocations of earlier trainers stay with
        # a process and slow later ones: tools/episode_cost.py)
        import subprocess
        for name in shapes:
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shapes", name,
                                  "--schedule", args.schedule, "--variants", args.variants] +
                                 [a for k, v in (("--steps", args.steps), ("--rounds", args.rounds),
                                                 ("--warmup", args.warmup), ("--age-steps", args.age_steps),
                                                 ("--stagger", args.stagger))
                                  for a in (k, str(v))])
            if rc:
                sys.exit(rc)
        return
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables_device, synthetic
    name = shapes[0]
    grid, P, R, E = SHAPES[name]
    lay = DeviceLayout(build_tables_device([synthetic(grid, grid, R)])[0], P)
    names = args.variants.split(",")
    if "off" not in names or any(k not in VARIANTS for k in names) or len(set(names)) != len(names):
        sys.exit(f"--variants: distinct names of {list(VARIANTS)} with off among them")
    trs = {k: build(lay, E, R, dict(VARIANTS[k], lagged_learn=args.schedule == "lagged"), args.age_steps,
                    args.stagger) for k in names}
    for tr in trs.values():
        block(tr, args.warmup)
    ms = {k: [] for k in names}
    for r in range(args.rounds):  # alternate, and rotate who goes first
        k0 = r % len(names)
        for k in names[k0:] + names[:k0]:
            ms[k].append(block(trs[k], args.steps))
    for tr in trs.values():
        tr.env.check_err()
        assert torch.isfinite(tr.last_loss).all()
    last = trs[names[-1]]
    ls = last.learn_summary() if last.learn_stats is not None else dict(steps=None, rows=None, rows_bad=None)
    vs = last.value_summary() if last.probe is not None else dict(probes=None, open=None, bias=None)
    mean = {k: float(np.mean(v)) for k, v in ms.items()}
    out = dict(shape=name, grid=grid, people=P, robots=R, envs=E, batch=E, schedule=args.schedule, replay="uniform",
               steps_per_block=args.steps, rounds=args.rounds, warmup=args.warmup,
               ms_per_step={k: [round(x, 4) for x in v] for k, v in ms.items()},
               mean={k: round(v, 4) for k, v in mean.items()},
               min={k: round(min(v), 4) for k, v in ms.items()}, max={k: round(max(v), 4) for k, v in ms.items()},
               built_in_order=names,
               delta_ms={k: round(mean[k] - mean["off"], 4) for k in names if k != "off"},
               per_round_delta_ms={k: [round(b - a, 4) for a, b in zip(ms["off"], ms[k])]
                                   for k in names if k != "off"},
               window=dict(of=names[-1], learn_steps=ls["steps"], rows=ls["rows"], rows_bad=ls["rows_bad"],
                           probes=vs["probes"], open=vs["open"], bias=vs["bias"]),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
