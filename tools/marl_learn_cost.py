"""Time VecTrainer.learn() for per-robot / QMIX nets with device events.

Shape: synthetic(128, 128, 16), 2276 people, 2048 envs, batch 16 * 2048. The trainer runs 4 steps
(the ring then holds 4 pushes), 20 warm-up learn steps, then 3 blocks of STEPS learn steps, each
between two device events; one JSON line with the blocks' ms per learn step.

usage: python tools/marl_learn_cost.py TREE NETS OPTS [STEPS]
  TREE   a checkout that holds dqn-marl_amd with its library built ('.': this one; another
         checkout, e.g. of the parent commit, to compare against -- run the two alternately)
  NETS   per_robot | qmix
  OPTS   off | dq (double_q) | nstep (n_step = 3) | on (double_q, Huber, target_tau = 0.01, n_step = 3)
"""
import json
import os
import sys

tree, nets, opts = sys.argv[1], sys.argv[2], sys.argv[3]
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 200
sys.path.insert(0, os.path.join(os.path.abspath(tree), "dqn-marl_amd"))

import torch  # noqa: E402
import evacx  # noqa: E402
from evacx.env import DeviceLayout  # noqa: E402
from evacx.layout import build_tables, synthetic  # noqa: E402
import evacx.trainer as trainer  # noqa: E402

R, E = 16, 2048
kw = dict(off={}, dq=dict(double_q=True), nstep=dict(n_step=3),
          on=dict(double_q=True, loss="huber", huber_delta=10.0, target_tau=0.01, n_step=3))[opts]
lay = DeviceLayout(build_tables(synthetic(128, 128, R)), 2276)
# (a checkout from before MultiAgentTrainer has VecTrainer only; options off is the same path)
cls = trainer.MultiAgentTrainer if kw else trainer.VecTrainer
tr = cls(lay, E, batch=16 * 2048, replay_capacity=1 << 18, nets=nets, learner_seed=1, target_every=1 << 30, **kw)
for _ in range(4):
    tr.step()
tr.sync()
torch.cuda.synchronize()
for _ in range(20):
    tr.learn()
torch.cuda.synchronize()
blocks = []
for _ in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.learn()
    e1.record()
    torch.cuda.synchronize()
    blocks.append(e0.elapsed_time(e1) / steps)
print(json.dumps(dict(tree=os.path.dirname(evacx.__file__), nets=nets, opts=opts, steps=steps,
                      ms_per_learn=[round(x, 4) for x in blocks],
                      loss_finite=bool(torch.isfinite(tr.last_loss).all()) if tr.last_loss is not None else None)),
      flush=True)
