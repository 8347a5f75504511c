"""Vectorised multi-agent DQN training loop, fully device-resident.

One ``step()`` = for all E envs x R robots of this rank:
  act      -- expand the compact observations, Q-forward (dropout active, as the
              reference's act never leaves train mode), epsilon-greedy (evx_act)
  env.step -- evx_env_step (the CA, bit-exact with the reference's step)
  push     -- E*R transitions into the replay ring (team reward/done per env)
  learn    -- sample B, online + target forwards, TD loss, backward, optional
              gradient all-reduce (RCCL over xGMI when world > 1), clip + Adam
  reset    -- auto-reset of finished envs (reference reset semantics) fused into
              the env.step launch; the heavy-first dispatch order of the next
              env.step and the next act's env order (evx_env_orders) follow it in
              one launch on the same stream
With groups > 1 the envs are split into parts that run act -> env.step -> push on
their own streams, so one part's env.step tail overlaps the others' work.

Reference: runners/train_double_dqn.py:43-69 (independent robots, shared team
reward) generalised to R robots and E envs; DQNAgent.act/remember/learn
(agents/dqn_agent.py:97-168). No host syncs inside ``step()``.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from ._lib import OBS_WORDS, check, evx_replay, lib
from .env import DeviceLayout, VecEnv, _check_out_rows, _ptr, _stream, n_layout_rows
from .qmlp import act_ws_ints
from .qnet import DROPOUT_P, Learner, validate_nets_options, validate_td_options


class Replay:
    """Uniform replay ring of compact observations in HBM."""

    def __init__(self, capacity: int, device):
        self.capacity = int(capacity)
        i32 = dict(dtype=torch.int32, device=device)
        self.s = torch.zeros(self.capacity * OBS_WORDS, **i32)
        self.s2 = torch.zeros(self.capacity * OBS_WORDS, **i32)
        self.a = torch.zeros(self.capacity, **i32)
        self.r = torch.zeros(self.capacity, dtype=torch.float32, device=device)
        self.done = torch.zeros(self.capacity, dtype=torch.uint8, device=device)
        self.c = evx_replay(capacity=self.capacity, s=self.s.data_ptr(), s2=self.s2.data_ptr(), a=self.a.data_ptr(),
                            r=self.r.data_ptr(), done=self.done.data_ptr())
        self.pos = 0
        self.size = 0

    def push(self, s, s2, a, r_env, done_env, n, agents_per_env, s2_term=None):
        """s2_term: terminal observations of auto-reset envs (taken where done_env)."""
        if s2_term is None:
            check(lib().evx_replay_push(C.byref(self.c), s.data_ptr(), s2.data_ptr(), a.data_ptr(), r_env.data_ptr(),
                                        done_env.data_ptr(), n, agents_per_env, self.pos, _stream()), "replay_push")
        else:
            check(lib().evx_replay_push_term(C.byref(self.c), s.data_ptr(), s2.data_ptr(), s2_term.data_ptr(),
                                             a.data_ptr(), r_env.data_ptr(), done_env.data_ptr(), n, agents_per_env,
                                             self.pos, _stream()), "replay_push_term")
        self.pos = (self.pos + n) % self.capacity
        self.size = min(self.capacity, self.size + n)

    def push_orders(self, env, perm, s, s2, a, r_env, done_env, n, agents_per_env, s2_term=None, sample=None):
        """push with env's next dispatch order and act env order (perm) in the same launch
        (evx_env_orders_push_sample; power-of-two capacity). sample = (B, seed, offset, out): also
        draw the learn step's batch into out, as sample() would right after the push."""
        size = min(self.capacity, self.size + n)
        B, seed, offset, out = sample if sample is not None else (0, 0, 0, None)
        o = (lambda k: out[k].data_ptr()) if out is not None else (lambda k: None)
        check(lib().evx_env_orders_push_sample(
            C.byref(env.lay.c), C.byref(env.c), _ptr(perm), C.byref(self.c), s.data_ptr(), s2.data_ptr(),
            _ptr(s2_term), a.data_ptr(), r_env.data_ptr(), done_env.data_ptr(), n, agents_per_env, self.pos,
            B, size, seed, offset, o("s"), o("s2"), o("a"), o("r"), o("done"), _stream()), "env_orders_push_sample")
        self.pos = (self.pos + n) % self.capacity
        self.size = size

    def window(self, n_next):
        """(base, count): the entries already in the ring that a push of n_next
        transitions does not overwrite -- the newest min(size, capacity - n_next)."""
        count = min(self.size, self.capacity - n_next)
        return (self.pos - count) % self.capacity, count

    def sample_window(self, base, count, B, seed, offset, out):
        check(lib().evx_replay_sample_window(C.byref(self.c), base, count, B, seed, offset, out["s"].data_ptr(),
                                             out["s2"].data_ptr(), out["a"].data_ptr(), out["r"].data_ptr(),
                                             out["done"].data_ptr(), _ptr(out.get("idx")), _stream()),
              "replay_sample_window")

    def sample(self, B, seed, offset, out):
        check(lib().evx_replay_sample(C.byref(self.c), self.size, B, seed, offset, out["s"].data_ptr(),
                                      out["s2"].data_ptr(), out["a"].data_ptr(), out["r"].data_ptr(),
                                      out["done"].data_ptr(), _ptr(out.get("idx")), _stream()), "replay_sample")

    def sample_agents(self, B, nets, seed, offset, out, joint=False):
        """Agent g's B draws from its own transitions, or (joint) the env-steps of one permutation for
        every agent, into rows [g B, (g + 1) B) of out (evx_replay_sample_agents / _sample_joint)."""
        fn = lib().evx_replay_sample_joint if joint else lib().evx_replay_sample_agents
        check(fn(C.byref(self.c), self.size, B, nets, seed, offset, out["s"].data_ptr(), out["s2"].data_ptr(),
                 out["a"].data_ptr(), out["r"].data_ptr(), out["done"].data_ptr(), _stream()),
              "replay_sample_agents/joint")

    def live_range(self):
        """(base, count) of the whole ring in push order, oldest first."""
        return (self.pos - self.size) % self.capacity, self.size

    def sample_nstep_agents(self, B, nets, seed, offset, base, count, stride, n_step, gamma, out, joint=False):
        """sample_agents' draws, each followed along its agent's chain as nstep does, in one launch
        (evx_replay_sample_nstep_agents); out["nlen"] (int32, L) and out["idx"] (int64, j0) are optional."""
        _check_out_rows("sample_nstep_agents", out, ("s", "s2", "a", "r", "done", "gamma_row"), nets * B,
                       f"needs {nets * B}", optional=("nlen", "idx"))
        check(lib().evx_replay_sample_nstep_agents(
            C.byref(self.c), self.size, B, nets, int(joint), seed, offset, base, count, stride, n_step, float(gamma),
            out["s"].data_ptr(), out["s2"].data_ptr(), out["a"].data_ptr(), out["r"].data_ptr(),
            out["done"].data_ptr(), out["gamma_row"].data_ptr(), _ptr(out.get("nlen")), _ptr(out.get("idx")),
            _stream()), "replay_sample_nstep_agents")

    def nstep(self, idx, B, base, count, stride, n_step, gamma, out):
        """n-step rows of the sampled slots idx (int64 [B], the samplers' idx_out) over the live
        range [base, base + count) mod capacity, stride rows pushed per env step
        (evx_replay_nstep): out["r"] = the discounted return of up to n_step rewards, out["s2"] /
        out["done"] = the chain's last slot's, out["gamma_row"] = gamma^L (f32 products),
        out["nlen"] (optional, int32) = L. The chain stops at a terminal slot and at the end of
        the range."""
        _check_out_rows("nstep", out, ("r", "done", "gamma_row", "s2"), B, f"B = {B}")
        if idx.dtype != torch.int64 or idx.numel() < B:
            raise ValueError(f"nstep: idx must be an int64 tensor of at least B = {B} elements")
        _check_out_rows("nstep", out, (), B, f"B = {B}", optional=("nlen",))  # (after idx, as it always was)
        nlen = out.get("nlen")
        check(lib().evx_replay_nstep(C.byref(self.c), idx.data_ptr(), B, base, count, stride, n_step,
                                     float(gamma), out["s2"].data_ptr(), out["r"].data_ptr(),
                                     out["done"].data_ptr(), out["gamma_row"].data_ptr(), _ptr(nlen),
                                     _stream()), "replay_nstep")


class _Group:
    """One part of the envs with its own stream chain (act -> env.step -> push): with
    several groups, one group's env.step launch tail (its heaviest envs, few waves)
    overlaps the other groups' act and env.step instead of idling the chip."""

    def __init__(self, env: VecEnv, g: int, row0: int, actions: torch.Tensor, device):
        self.env, self.g, self.row0 = env, g, row0
        self.n = env.E * env.lay.R
        self.actions = actions  # this group's rows of the trainer's action buffer
        # act, env.step, push on a high-priority stream: the learn stream's workgroups
        # then fill the env launch's tail instead of competing for its first slots
        self.main = torch.cuda.Stream(device=device, priority=-1)
        # one group: the next step's orders (evx_env_orders) beside the learn; extra resets
        self.side = torch.cuda.Stream(device=device, priority=0)
        cur = torch.cuda.current_stream(device)
        self.ev_push = torch.cuda.Event()
        self.ev_push.record(cur)
        self.ev_act = torch.cuda.Event()
        self.ev_order = torch.cuda.Event()
        self.ev_order.record(cur)
        self.perm = None  # the act's env order over this group's envs (x3 table path), or None
        self.act_ws = None  # the x3 act's workspace (evx_qmlp_fwd_out.act_ws), made at the first act
        self.ep = None  # this group's envs of the trainer's EpisodeStats (episode_stats=True), or None
        self.probe = None  # this group's envs of the trainer's ValueProbe (value_probe=True), or None
        self.q = None  # value_probe: this group's rows of the act's Q output [n][5]


class VecTrainer:
    # per-robot / QMIX nets with double_q / loss / huber_delta / target_tau / n_step: MultiAgentTrainer
    agent_options = False

    def __init__(self, layout: DeviceLayout, E: int, seed_base: int = 1234, env_offset: int = 0,
                 kind: str = "mlp", precision: str = "f32", batch: int = 4096, replay_capacity: int = 1 << 20,
                 lr: float = 1e-4, gamma: float = 0.99, epsilon: float = 1.0, epsilon_min: float = 0.02,
                 epsilon_decay: float = 0.9995, target_every: int = 1000, learner_seed: int = 0,
                 grad_hook=None, learn_every: int = 1, lagged_learn: bool = False, replay: str = "uniform",
                 prio_alpha: float = 0.6, prio_beta0: float = 0.4, prio_beta_steps: int = 100000,
                 prio_eps: float = 1e-6, groups: int = 1, layout_of=None, world_envs: Optional[int] = None,
                 nets: str = "shared", act_table: Optional[bool] = None, episode_stats: bool = False,
                 double_q: bool = False, loss: str = "mse", huber_delta: float = 1.0, target_tau: float = 0.0,
                 n_step: int = 1, learn_stats: bool = False, value_probe: bool = False):
        """groups: the envs are split into this many parts, each stepping on its own
        stream chain (see _Group), group g's act after group g - 1's (it overlaps that
        group's env.step); neither the env results nor the act's dropout masks (one stream
        per step, rows keyed by global agent id) depend on it.
        layout: a DeviceLayout, or an evacx.env.LayoutSet with layout_of = each env's
        layout (per-env layouts; observations in the replay carry their layout).
        world_envs: envs over all ranks (default E). This rank's envs are global ids
        env_offset .. env_offset + E - 1; the act's epsilon draws and dropout rows are keyed
        by global agent id, so every env's trajectory is the same at any GPU count as long
        as the actions do not depend on the (rank-shared) weights' history.
        nets: "shared" (one Q-network for every robot) or "per_robot" (robot r of every env has
        its own network, memory and optimizer, as runners/train_double_dqn.py:35-56 gives each
        robot its own DQNAgent: evacx.qgroup.GroupedLearner, batch / R transitions per net per
        learn step, strict schedule, one GPU) or "qmix" (per-robot nets under a QMIX mixer,
        runners/train_qmix.py: batch / R joint env-steps per learn step, evacx.qgroup.GroupedQMix).
        episode_stats: keep every env's episode returns, lengths and evacuated / dead counts on
        the device (evacx.episodes.EpisodeStats: one more launch per group and step on the
        group's stream, between env.step and the push; no host sync) for episode_summary().
        Off: nothing is allocated or launched for it.
        double_q / loss ("mse", "huber") / huber_delta / target_tau: the learner's TD options
        (evacx.qnet.Learner); target_tau > 0 replaces the hard copy every target_every learn steps
        by Learner.soft_update() after every learn step. nets="shared" here; the subclass
        MultiAgentTrainer takes them for the other two: with nets="per_robot" every robot's net
        takes them (GroupedLearner.learn_obs / soft_update); with "qmix" Double-Q selects every
        agent's bootstrap action, the Huber loss acts on the mixed TD error and the soft update
        covers the agents and the target mixer (GroupedQMix).
        n_step > 1: the learn step turns its sampled slots into n-step rows (Replay.nstep, one more
        launch after the sampler's, on its stream: r = the discounted return of up to n_step
        rewards of the same env and robot, s2 / done the chain's last slot's, the discount per row
        in samp["gamma_row"], the chain lengths in samp["nlen"]); under every sampler and both
        schedules. nets="per_robot" / "qmix" (MultiAgentTrainer only): the sampler and the chains in one launch
        (evx_replay_sample_nstep_agents over the whole ring), gamma_row [R][batch / R]; QMIX reads
        agent 0's rows, the joint rows'. groups=1 and no step(extra_reset=...). 1: nothing of it runs.
        learn_stats: the learner folds every learn step's batch into an evacx.lstats.LearnStats (two
        launches after clip + Adam, on its stream) for learn_summary(); nets="shared" (1 net) or
        "per_robot" (R nets), not "qmix" (the target there is the mixer's).
        value_probe: the act also writes its Q rows, and an evacx.lstats.ValueProbe pairs the Q of
        the actions taken at every episode's first step with the episode's discounted return (one
        more launch per group and step, where the episode statistics' runs) for value_summary();
        every nets mode. Both off: nothing is allocated or launched for them; on, the training
        itself is the same bit for bit."""
        if learn_stats and nets == "qmix":  # (before anything reads the layout)
            raise ValueError("learn_stats needs nets='shared' or 'per_robot': the QMIX target is the mixer's")
        validate_td_options(loss, huber_delta, target_tau)
        self.target_tau = float(target_tau)
        if precision not in ("f32", "bf16", "exact"):
            raise ValueError(f"precision must be 'f32', 'bf16' or 'exact', not {precision!r}")
        validate_nets_options(nets, R=layout.R, E=E, batch=batch, replay_capacity=replay_capacity, n_step=n_step,
                              groups=groups, kind=kind, precision=precision, lagged_learn=lagged_learn, replay=replay,
                              per_env_layouts=layout_of is not None, grad_hook=grad_hook is not None,
                              td_options=bool(double_q or loss != "mse" or huber_delta != 1.0 or target_tau != 0.0),
                              agent_options=self.agent_options)
        self.n_step = n_step
        self.last_range = None  # n_step > 1: the (base, count) the last learn step's chains ran over
        # a ring smaller than one push: two rows of the push would share a slot (the winner undefined)
        # and window() would count a negative number of entries. Groups push their own rows one after
        # the other; the lagged schedule's window sets a whole step's rows aside
        n_groups = groups if isinstance(groups, int) and groups > 1 and not lagged_learn else 1
        push_rows = -(-E // n_groups) * layout.R
        if replay_capacity < push_rows:
            raise ValueError(f"replay_capacity = {replay_capacity} is smaller than one push of {push_rows} rows "
                             f"(E * R / groups = {E} * {layout.R} / {n_groups})")
        self.lay, self.E, self.R = layout, E, layout.R
        self.device = layout.device
        # the push reads env.obs_prev: no copy per step
        self.env = VecEnv(layout, E, obs_buffers=2, layout_of=layout_of)
        self.env.seed([seed_base + env_offset + i for i in range(E)])
        self.env.reset()
        parts = self.env.split(groups) if groups > 1 else [self.env]
        self.per_robot = nets in ("per_robot", "qmix")
        # per-robot / QMIX nets: the options as the grouped learn steps take them (None / 0: off, and
        # then the entries and launches of a trainer without them)
        self.double_q = bool(double_q)
        self.huber = float(huber_delta) if loss == "huber" else 0.0
        if self.per_robot:
            from .qgroup import GroupedLearner, GroupedQMix
            self.learn_stats = None
            if learn_stats:
                from .lstats import LearnStats
                self.learn_stats = LearnStats(self.R, self.device)
            self.glearner = GroupedLearner(self.R, self.device, lr=lr, gamma=gamma, seed=learner_seed,
                                           stats=self.learn_stats)
            # qmix: the R robots of an env are the agents of runners/train_qmix.py -- joint samples
            # (the same env-steps for every agent), the mixer's loss over the team reward
            self.qmix = GroupedQMix(self.glearner, seed=learner_seed) if nets == "qmix" else None
        # precision: "f32" -- f32-accurate x3 (the fused MLP kernels; the conv net's implicit-GEMM
        # convolutions, bf16 hi/lo operand pairs); "bf16"; "exact" -- every product on the exact-f32
        # MFMA GEMMs (evx_gemm f32, no fused kernels: the golden-test path, either kind)
        lprec = "x3" if (kind == "conv" and precision == "f32") else precision
        if not self.per_robot:
            self.learn_stats = None
            if learn_stats:
                from .lstats import LearnStats
                self.learn_stats = LearnStats(1, self.device)
        self.learner = Learner(kind=kind, device=self.device, lr=lr, gamma=gamma, precision=lprec,
                               seed=learner_seed, double_q=double_q, loss=loss, huber_delta=huber_delta,
                               target_tau=target_tau, stats=self.learn_stats) if not self.per_robot else None
        # the arithmetic the Q-network actually runs: "x3" (f32 operands as bf16 hi + lo pairs on the
        # bf16 MFMA, f32 accumulation: f32 within the tests' stated tolerances), "f32" (exact f32
        # MFMA) or "bf16" -- read from what the learner built
        if self.per_robot:
            self.q_arith = "x3"
        elif self.learner.fast is not None:
            self.q_arith = "x3" if self.learner.fast.x3 else "bf16"
        else:
            self.q_arith = {"exact": "f32"}.get(lprec, lprec)
        if self.learner is not None:
            self.learner.grad_hook = grad_hook
        # replay: "uniform" (DQNAgent.memory's random.sample) or "prioritized" (evacx.prio:
        # device sum/min trees, importance-weighted loss, beta annealed to 1)
        self.prio = replay == "prioritized"
        if self.prio:
            from .prio import PrioReplay
            self.replay = PrioReplay(replay_capacity, self.device, alpha=prio_alpha, eps=prio_eps)
        elif replay == "uniform":
            self.replay = Replay(replay_capacity, self.device)
        else:
            raise ValueError(f"replay must be 'uniform' or 'prioritized', not {replay!r}")
        self.prio_beta0, self.prio_beta_steps = prio_beta0, prio_beta_steps
        self.batch = batch
        self.epsilon, self.epsilon_min, self.epsilon_decay = epsilon, epsilon_min, epsilon_decay
        self.target_every, self.learn_every = target_every, learn_every
        # lagged_learn: learn step t samples the transitions pushed up to step t-1 and runs
        # on its own stream concurrently with env.step t (see step())
        self.lagged = lagged_learn
        n = E * self.R
        self.n_agents = n
        self.agent0 = env_offset * self.R  # global agent id of this rank's first robot
        self.n_world = (E if world_envs is None else int(world_envs)) * self.R
        if self.agent0 % 2:
            raise ValueError("env_offset * R must be even (dropout hash rows come in pairs)")
        self.actions = torch.zeros(n, dtype=torch.int32, device=self.device)
        ng = n // len(parts)
        self.groups: List[_Group] = [_Group(p, g, g * ng, self.actions[g * ng:(g + 1) * ng], self.device)
                                     for g, p in enumerate(parts)]
        self.main = self.groups[0].main
        # episode statistics (the reference's per-episode log, runners/train_dqn.py:129-161), or None
        self.episodes = None
        if episode_stats:
            from .episodes import EpisodeStats
            self.episodes = EpisodeStats(E, self.device, layout.P, layout_idx=self.env.layout_idx,
                                         n_layouts=n_layout_rows(layout))
            for grp in self.groups:
                grp.ep = self.episodes.view(grp.g * grp.env.E, grp.env.E) if len(parts) > 1 else self.episodes
        # the value probe (evacx.lstats.ValueProbe) and the act's Q rows it reads, or None
        self.probe = self.act_q = None
        if value_probe:
            from .lstats import ValueProbe
            self.probe = ValueProbe(E, self.R, self.device, gamma, layout_idx=self.env.layout_idx,
                                    n_layouts=n_layout_rows(layout))
            self.act_q = torch.zeros(E * self.R * 5, dtype=torch.float32, device=self.device)
        for grp in self.groups:
            if self.probe is not None:
                grp.probe = self.probe.view(grp.g * grp.env.E, grp.env.E) if len(parts) > 1 else self.probe
                grp.q = self.act_q[grp.row0 * 5:(grp.row0 + grp.n) * 5]
        self.samp = dict(s=torch.zeros(batch * OBS_WORDS, dtype=torch.int32, device=self.device),
                         s2=torch.zeros(batch * OBS_WORDS, dtype=torch.int32, device=self.device),
                         a=torch.zeros(batch, dtype=torch.int32, device=self.device),
                         r=torch.zeros(batch, dtype=torch.float32, device=self.device),
                         done=torch.zeros(batch, dtype=torch.uint8, device=self.device))
        if self.prio:
            self.samp.update(idx=torch.zeros(batch, dtype=torch.int64, device=self.device),
                             w=torch.zeros(batch, dtype=torch.float32, device=self.device),
                             td=torch.zeros(batch, dtype=torch.float32, device=self.device))
        if self.n_step > 1:  # the samplers' slot indices, the rows' discounts and chain lengths
            if not self.prio:
                self.samp["idx"] = torch.zeros(batch, dtype=torch.int64, device=self.device)
            self.samp.update(gamma_row=torch.zeros(batch, dtype=torch.float32, device=self.device),
                             nlen=torch.zeros(batch, dtype=torch.int32, device=self.device))
        # replay sampling: per rank (each rank samples its own shard); act draws: one key for
        # all ranks (counters are global agent ids)
        self.seed = learner_seed * 7919 + env_offset + 17
        self.act_seed = learner_seed * 7919 + 17
        self.t = 0
        self.learn_steps = 0
        cur = torch.cuda.current_stream(self.device)
        self.ev_reset = torch.cuda.Event()
        self.ev_reset.record(cur)
        self.reset_pending = False
        self.join_caller = True  # the first step waits for the caller's stream (set-up work)
        self._orders_side = False  # the last step's orders were made on the side stream (act waits for them)
        self._presampled = False   # this step's learn batch was drawn by the push launch
        self.lstream = torch.cuda.Stream(device=self.device, priority=0)
        self.ev_learned = torch.cuda.Event()
        self.ev_learned.record(cur)
        # prioritized replay, strict schedule: the priority update of learn t runs on its own stream
        # beside clip+Adam, the act and env.step of t + 1 (nothing there reads the trees); the next
        # expose / sample waits for it, so the trees see the same operations in the same order
        self.pstream = torch.cuda.Stream(device=self.device, priority=0)
        self.ev_td = torch.cuda.Event()
        self.ev_prio = torch.cuda.Event()
        self.ev_prio.record(cur)
        self.last_loss: Optional[torch.Tensor] = None
        # bf16 MLP: act and learn straight from compact observations (csrc/qmlp.hip)
        self.fast = self.learner.fast if self.learner is not None else None
        if self.fast is None:
            self.lagged = False  # the lagged schedule's two-phase learn needs the fused MLP path
        self._perm = None
        if act_table is None:
            act_table = True
        if self.fast is not None and self.fast.x3 and layout_of is None and act_table:
            # act fast path: envs past the fire's last step start fc1 from a per-centre table of the
            # static features' contribution (rebuilt with every weight update) and add only the
            # occupancy columns; the act visits those envs first (VecEnv.act_perm) so its row tiles
            # are uniform. x3 only (the table replaces ~3/4 of fc1's products); bf16: off (the
            # rebuild costs what the act saves, tools/gpu_ab_static.sh)
            lc = self.lay.c  # centres only where robots can be (Map.robot_range): 55 of 130 columns at cfg3
            xr = (max(lc.rx_lo, 0), min(lc.rx_hi, lc.L + 1))
            self.fast.attach_static(lc, lc.L, lc.W, lc.t_max, x_range=xr)
            # the target net's table too (rebuilt at each target sync): on the learner's routes
            # through the act kernels (MLPFast.forward_pair_plan says which batch takes which) the
            # target forward starts fc1 from it for replay rows past the fire's last step
            self.learner.fast_t.attach_static(lc, lc.L, lc.W, lc.t_max, x_range=xr)
            # the act's env order, per group (each group's act visits its own envs)
            self._perm = torch.zeros(E, dtype=torch.int32, device=self.device)
            for grp in self.groups:
                grp.perm = self._perm[grp.g * grp.env.E:(grp.g + 1) * grp.env.E]
        for grp in self.groups:  # the first step's orders (the reset wrote every class byte)
            grp.env.compute_orders(perm=grp.perm)

    def _act(self, grp: _Group):
        """DQNAgent.act in train mode for one group's robots: dropout active, epsilon-greedy
        over argmax Q; the epsilon draws are counted over all E*R robots of the step."""
        g0 = self.agent0 + grp.row0  # global agent id of the group's first robot
        off = self.t * self.n_world + g0
        if self.per_robot:  # robot r of every env through net r, one launch
            self.glearner.act(self.lay.c, grp.env.obs, grp.env.E, actions=grp.actions, q=grp.q,
                              epsilon=float(self.epsilon), act_seed=self.act_seed, act_offset=off)
            return
        if self.fast is not None:  # one mask stream per step (act_streams), rows keyed by global agent id
            if grp.act_ws is None and act_ws_ints(grp.n) > 0:  # the persistent act's list of tiles off the table path
                grp.act_ws = torch.zeros(act_ws_ints(grp.n), dtype=torch.int32, device=self.device)
            self.fast.act(self.lay.c, grp.env.obs, grp.n,
                          drop=(self.learner.seed, self.learner.drop_stream, DROPOUT_P, None, g0),
                          q=grp.q, actions=grp.actions, epsilon=float(self.epsilon), act_seed=self.act_seed,
                          act_offset=off, perm=grp.perm, rows_per_env=0 if grp.perm is None else self.R, ws=grp.act_ws)
            return
        x = grp.env.expand_obs(torch.float32)  # [E/G, R, 11, 11, 6]
        # per-group scratch: the groups' acts run concurrently on their own streams
        Q = self.learner.q_values(x.view(grp.n, 11, 11, 6), train=True, tag=f"act{grp.g}" if grp.g else "act")
        check(lib().evx_act(Q.data_ptr(), grp.n, self.learner.actions, float(self.epsilon), self.act_seed, off,
                            grp.actions.data_ptr(), _stream()), "act")
        if grp.q is not None:  # the probe's Q rows (the forward's scratch is rewritten by the next act)
            grp.q.copy_(Q.reshape(-1))

    def _act_stream(self):
        """A fresh dropout mask stream for this step's act: every group's act draws from it (rows keyed
        by global agent id), so the masks do not depend on the group count."""
        if self.fast is not None and not self.per_robot:
            self.learner.drop_stream += 1

    def act(self):
        """Launch DQNAgent.act for every robot of every env on the trainer's stream and return
        the actions buffer. The kernels run asynchronously: read the returned tensor only after
        sync() (or on a stream that waits for the trainer's), since the next step overwrites it."""
        self._act_stream()
        for grp in self.groups:
            self._act(grp)
        return self.actions

    def learn(self, window=None, phase: str = "all"):
        """window: (base, count) of the replay ring to sample from (default: all of it).
        phase: "all", or "grads" (sample .. backward) then "update" (clip+Adam, bf16
        repack, epsilon, target sync) -- the update may wait for readers of the weights."""
        if self.per_robot:  # every robot's net on batch / R of its own transitions
            Bn = self.batch // self.R
            if self.replay.size < self.batch:
                return None
            sp = self.samp
            grow = None
            if self.n_step > 1:
                # the draws of the sampler below, each followed along its robot's chain over the whole
                # ring in the same launch (evx_replay_sample_nstep_agents; one push is E * R rows)
                self.last_range = self.replay.live_range()
                self.replay.sample_nstep_agents(Bn, self.R, self.seed + 1, self.learn_steps * self.batch,
                                                self.last_range[0], self.last_range[1], self.n_agents, self.n_step,
                                                self.glearner.gamma, sp, joint=self.qmix is not None)
                grow = sp["gamma_row"]  # [R][Bn]; QMIX reads agent 0's rows [0, Bn): the joint rows'
            else:
                self.replay.sample_agents(Bn, self.R, self.seed + 1, self.learn_steps * self.batch, sp,
                                          joint=self.qmix is not None)
            if self.qmix is not None:  # agent 0's rows carry the team reward / done of the sampled env-steps
                loss = self.qmix(self.lay.c, sp["s"], sp["a"], sp["r"], sp["done"], sp["s2"], Bn,
                                 double_q=self.double_q, huber_delta=self.huber, gamma_row=grow)
            else:
                loss = self.glearner.learn_obs(self.lay.c, sp["s"], sp["a"], sp["r"], sp["done"], sp["s2"], Bn,
                                               gamma_row=grow, double_q=self.double_q,
                                               huber_delta=[self.huber] * self.R if self.huber else None)
            self._learned()
            return loss
        if phase != "update":
            if (self.replay.size if window is None else window[1]) < self.batch:
                return None
            w = td = None
            if self.prio:
                # the trees only hold exposed slots: the window is implicit (hidden slots have 0 mass)
                beta = min(1.0, self.prio_beta0 + (1.0 - self.prio_beta0) * self.learn_steps / self.prio_beta_steps)
                w, td = self.samp["w"], self.samp["td"]
                torch.cuda.current_stream(self.device).wait_event(self.ev_prio)  # (free once it has run)
                self.replay.sample_prio(self.batch, beta, self.seed + 1, self.learn_steps * self.batch, self.samp,
                                        self.samp["idx"], w)
            elif window is None:
                if not self._presampled:  # (drawn by the push launch of this step)
                    self.replay.sample(self.batch, self.seed + 1, self.learn_steps * self.batch, self.samp)
                self._presampled = False
            else:
                self.replay.sample_window(window[0], window[1], self.batch, self.seed + 1,
                                          self.learn_steps * self.batch, self.samp)
            grow = None
            if self.n_step > 1:
                # the sampled slots' n-step rows over the range the batch was drawn from (lagged: the
                # window, which the concurrent push does not write), in place of their r / done / s2
                self.last_range = window if window is not None else self.replay.live_range()
                self.replay.nstep(self.samp["idx"], self.batch, self.last_range[0], self.last_range[1],
                                  self.n_agents, self.n_step, self.learner.gamma, self.samp)
                grow = self.samp["gamma_row"]
            side_prio = self.prio and phase == "all" and self.fast is not None and not self.lagged
            if self.fast is not None:
                loss = self.learner.learn_obs(self.lay.c, self.samp["s"], self.samp["a"], self.samp["r"],
                                              self.samp["done"], self.samp["s2"], self.batch,
                                              update=phase == "all" and not side_prio, weights=w, td_abs=td,
                                              gamma_row=grow)
            else:
                assert phase == "all", "a two-phase learn needs the fused MLP path"
                s = self.env.expand_obs(torch.float32, self.samp["s"]).view(self.batch, 11, 11, 6)
                s2 = self.env.expand_obs(torch.float32, self.samp["s2"]).view(self.batch, 11, 11, 6)
                loss = self.learner.learn(s, self.samp["a"], self.samp["r"], self.samp["done"], s2, weights=w,
                                          td_abs=td, gamma_row=grow)
            if side_prio:  # |TD| is ready: the trees' update on the priority stream, then clip+Adam here
                cur = torch.cuda.current_stream(self.device)
                self.ev_td.record(cur)
                with torch.cuda.stream(self.pstream):
                    self.pstream.wait_event(self.ev_td)
                    self.replay.update(self.samp["idx"], td, self.batch)
                    self.ev_prio.record(self.pstream)
                self.learner.step_optimizer()
            elif self.prio:
                self.replay.update(self.samp["idx"], td, self.batch)
            if phase == "grads":
                return loss
        else:
            self.learner.step_optimizer()
            loss = self.learner.loss
        self._learned()
        return loss

    def _learned(self):
        """After every learn step: the step count, the epsilon schedule and the target nets."""
        self.learn_steps += 1
        if self.epsilon > self.epsilon_min:  # DQNAgent.learn epsilon schedule (agents/dqn_agent.py:163-164)
            self.epsilon *= self.epsilon_decay
        if self.target_tau > 0:  # Polyak targets after every learn step, no periodic hard copy
            if not self.per_robot:
                self.learner.soft_update()
            elif self.qmix is not None:
                self.qmix.soft_update(self.target_tau)
            else:
                self.glearner.soft_update([self.target_tau] * self.R)
        elif self.learn_steps % self.target_every == 0:
            if not self.per_robot:
                self.learner.sync_target()
            elif self.qmix is not None:
                self.qmix.sync_targets()
            else:
                self.glearner.sync_target()

    def step(self, extra_reset: Optional[torch.Tensor] = None, ev_env=None, ev_learn=None, ev_act=None):
        """One training step. Finished envs are reset inside the env.step launch
        (auto-reset: the reset of an env that ends runs in its own wave, in the shadow
        of the launch's heavy envs); the replay push takes their terminal observations.
        The heavy-first dispatch order of each group's next env.step and the next act's
        env order come from one launch over the class bytes the step wrote
        (evx_env_orders): one group on its side stream beside the push and the learn (the
        act waits for it, long complete by then), several groups on their own streams.
        extra_reset: bool [E] of further envs to reset (benchmark staggering, side
        stream); ev_env / ev_learn:
        optional (start, end) CUDA events (env: group 0's env.step); ev_act: group 0's act.

        Default order is the reference's (act, env.step, remember, learn). With
        lagged_learn the learn step runs on its own stream from the ring as it was
        before this step's push (minus the slots the push overwrites): its gradients
        overlap act and env.step, its weight update waits for every group's act to have
        read the weights, and the next acts wait for the update."""
        if extra_reset is not None and self.n_step > 1:
            raise ValueError("extra_reset with n_step > 1: a forced reset breaks a transition chain without a done")
        caller = torch.cuda.current_stream(self.device)
        join = self.join_caller
        if self.join_caller or extra_reset is not None:  # inputs made on the caller's stream
            for grp in self.groups:
                grp.main.wait_stream(caller)
            self.join_caller = False
        G = self.groups
        # one group, uniform replay, no warm-up reset: the push and the next step's orders in one launch
        # on the main stream (no side-stream event); otherwise the orders on the side stream
        fused = (len(G) == 1 and extra_reset is None and type(self.replay) is Replay
                 and (self.replay.capacity & (self.replay.capacity - 1)) == 0)
        reset_wait, self.reset_pending = self.reset_pending, False
        self._presampled = False
        self._act_stream()
        # act: every group on its own stream, after the previous update (lagged) or learn
        for grp in G:
            with torch.cuda.stream(grp.main):
                if reset_wait:  # a cross-stream wait costs a gap: only when there was a reset
                    grp.main.wait_event(self.ev_reset)
                if self.lagged or grp.g > 0:
                    grp.main.wait_event(self.ev_learned)
                if grp.g > 0:  # the acts run one after the other: act g overlaps env.step g - 1
                    grp.main.wait_event(G[grp.g - 1].ev_act)
                if len(G) == 1 and self._orders_side:  # the orders from the side stream
                    grp.main.wait_event(grp.ev_order)
                if ev_act is not None and grp.g == 0:
                    ev_act[0].record(grp.main)
                self._act(grp)
                if ev_act is not None and grp.g == 0:
                    ev_act[1].record(grp.main)
                if self.lagged or grp.g + 1 < len(G):  # read by the update / the next group's act
                    grp.ev_act.record(grp.main)
        if self.lagged:
            # learn t: gradients from the ring as it stood after push t-1 (minus the slots
            # push t overwrites), overlapping act t and env.step t; the weight update
            # waits until every act t has read the weights, and act t+1 waits for it
            win = self.replay.window(self.n_agents)
            do_learn = self.t % self.learn_every == 0 and win[1] >= self.batch and self.fast is not None
            with torch.cuda.stream(self.lstream):
                for grp in G:
                    self.lstream.wait_event(grp.ev_push)
                if ev_learn is not None:
                    ev_learn[0].record(self.lstream)
                if self.prio:  # push t-1 visible, the slots push t overwrites hidden
                    self.replay.expose(n_hide=self.n_agents)
                if do_learn:
                    self.learn(window=win, phase="grads")
                for grp in G:
                    self.lstream.wait_event(grp.ev_act)
                self.last_loss = self.learn(phase="update") if do_learn else None
                if ev_learn is not None:
                    ev_learn[1].record(self.lstream)
                self.ev_learned.record(self.lstream)
        # a cross-stream reader of the push: the lagged learn stream, group 0's learn, a reset
        for grp in G:
            with torch.cuda.stream(grp.main):
                if ev_env is not None and grp.g == 0:
                    ev_env[0].record(grp.main)
                grp.env.step(grp.actions, order=False, auto_reset=True)
                if ev_env is not None and grp.g == 0:
                    ev_env[1].record(grp.main)
                if grp.ep is not None:  # before this stream's next step overwrites reward / done / counts
                    grp.ep.update(grp.env.reward, grp.env.done, grp.env.counts)
                if grp.probe is not None:  # before this stream's next act overwrites its Q rows
                    grp.probe.update(grp.q, grp.actions, grp.env.reward, grp.env.done)
                if fused:
                    # the strict schedule's learn batch drawn in the same launch (the ring after this push;
                    # not with n_step > 1: that draw leaves no slot indices)
                    smp = None
                    if (self.n_step == 1 and not self.lagged and not self.prio and not self.per_robot
                            and self.t % self.learn_every == 0
                            and min(self.replay.capacity, self.replay.size + grp.n) >= self.batch):
                        smp = (self.batch, self.seed + 1, self.learn_steps * self.batch, self.samp)
                    self.replay.push_orders(grp.env, grp.perm, grp.env.obs_prev, grp.env.obs, grp.actions,
                                            grp.env.reward, grp.env.done, grp.n, self.R, s2_term=grp.env.obs_term,
                                            sample=smp)
                    self._presampled = smp is not None
                else:
                    self.replay.push(grp.env.obs_prev, grp.env.obs, grp.actions, grp.env.reward, grp.env.done,
                                     grp.n, self.R, s2_term=grp.env.obs_term)
                if len(G) > 1:  # several groups: the orders on this stream, after the push
                    grp.env.compute_orders(perm=grp.perm)
                if not fused or self.lagged:  # read by the side stream / the lagged learn stream
                    grp.ev_push.record(grp.main)
        if extra_reset is not None:  # after every group's push, on group 0's side stream (warm-up only)
            side = G[0].side
            extra_reset.record_stream(side)  # the caller may free it before the side stream reads it
            with torch.cuda.stream(side):
                side.wait_stream(caller)
                for grp in G:
                    side.wait_event(grp.ev_push)
                mask = extra_reset & ~self.env.done.bool()
                self.env.reset(mask=mask)
                if self.episodes is not None:  # after every group's update (ev_push): their partial episodes end here
                    self.episodes.discard(mask)
                if self.probe is not None:  # their probes close without a pair
                    self.probe.discard(mask)
                if len(G) > 1:
                    for grp in G:  # the orders again, with the reset envs' new classes
                        grp.env.compute_orders(perm=grp.perm)
                self.ev_reset.record(side)
            self.reset_pending = True
        self._orders_side = len(G) == 1 and not fused
        if self._orders_side:
            # the next step's dispatch order and the next act's env order from the class bytes the
            # step (and a reset) just wrote, auto-reset envs included: one launch on the side stream,
            # beside the learn's first kernels
            grp = G[0]
            with torch.cuda.stream(grp.side):
                grp.side.wait_event(grp.ev_push)  # (after an extra reset: the same stream)
                grp.env.compute_orders(perm=grp.perm)
                grp.ev_order.record(grp.side)
        if not self.lagged:  # the reference's order: learn after every group's push, on group 0's stream
            m = G[0].main
            with torch.cuda.stream(m):
                for grp in G[1:]:
                    m.wait_event(grp.ev_push)
                if self.prio:
                    m.wait_event(self.ev_prio)  # the last learn's priority update (idx / td are rewritten next)
                    self.replay.expose()
                if ev_learn is not None:
                    ev_learn[0].record(m)
                if self.t % self.learn_every == 0:
                    self.last_loss = self.learn()
                if ev_learn is not None:
                    ev_learn[1].record(m)
                if len(G) > 1:
                    self.ev_learned.record(m)
        self._presampled = False
        self.t += 1

    def episode_summary(self, clear: bool = True) -> dict:
        """sync(), then the statistics of the episodes finished since the last clearing call
        (EpisodeStats.summary: episodes, return_mean / _std / _min / _max, length_mean, evac_rate,
        death_rate, per_layout rows for a LayoutSet). Waits for the device; not part of a step."""
        if self.episodes is None:
            raise RuntimeError("episode_summary: the trainer was made with episode_stats=False")
        self.sync()
        return self.episodes.summary(clear=clear)

    def learn_summary(self, clear: bool = True) -> dict:
        """sync(), then the learn-batch statistics of the learn steps since the last clearing call
        (LearnStats.summary). Waits for the device; not part of a step."""
        if self.learn_stats is None:
            raise RuntimeError("learn_summary: the trainer was made with learn_stats=False")
        self.sync()
        return self.learn_stats.summary(clear=clear)

    def value_summary(self, clear: bool = True) -> dict:
        """sync(), then the value probe's window (ValueProbe.summary: probes, bad, open, q0_mean,
        return_mean, bias, rmse, corr, err_min, err_max, per_layout). Waits for the device."""
        if self.probe is None:
            raise RuntimeError("value_summary: the trainer was made with value_probe=False")
        self.sync()
        return self.probe.summary(clear=clear)

    def sync(self):
        """Make the current stream wait for all work of the steps so far. step() runs on
        the trainer's own streams and does not join the caller's stream each step (a
        cross-stream round trip costs tens of microseconds); read results after sync()."""
        cur = torch.cuda.current_stream(self.device)
        for grp in self.groups:
            cur.wait_stream(grp.main)
            cur.wait_event(grp.ev_order)
        cur.wait_event(self.ev_reset)
        cur.wait_event(self.ev_learned)
        cur.wait_event(self.ev_prio)
        self.join_caller = True


class MultiAgentTrainer(VecTrainer):
    """VecTrainer for nets="per_robot" or "qmix" with the learner's options: double_q, loss,
    huber_delta, target_tau and n_step as VecTrainer's docstring states them for these modes.
    VecTrainer itself refuses them there, as it always has; everything else -- arguments, step(),
    learn(), the summaries -- is VecTrainer's, and with every option at its default the two classes
    train bit for bit alike."""
    agent_options = True

    def __init__(self, layout, E: int, nets: str = "qmix", **kw):
        if nets not in ("per_robot", "qmix"):
            raise ValueError(f"MultiAgentTrainer: nets must be 'per_robot' or 'qmix', not {nets!r}")
        super().__init__(layout, E, nets=nets, **kw)


def make_allreduce_hook(dist, world: int):
    """Average the flat gradient buffer over ranks (one collective per learn step)."""
    backend = dist.get_backend()

    def hook(flat):
        if backend == "nccl":
            dist.all_reduce(flat, op=dist.ReduceOp.AVG)
        else:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
            flat.div_(world)
    return hook
