"""Population training: K independent DQN learners over one VecEnv, every step in grouped launches.

What a result needs before it can be reported is the same run over several seeds and several
learning rates, discounts and exploration schedules (the reference's
runners/overnight_experiments.py runs them one after another). ``PopulationTrainer`` trains K members
in one process: member k owns envs [k E/K, (k + 1) E/K) -- rows [k N, (k + 1) N), N = (E / K) R, of
the observation, action and Q buffers -- has its own network (one net for all R robots of its envs,
as VecTrainer's shared net), target network, Adam moments, replay ring, learning rate, discount,
exploration schedule and target period, and shares every launch with the others:

  act      evx_qmlp_act_gb            net k on its row block, epsilon[k], one launch
  env.step evx_env_step               all E envs with auto-reset, one launch (+ EpisodeStats.update)
  push     evx_replay_push_blocks     row k N + i -> ring k, slot (pos + i) mod C, one launch
  orders   evx_env_orders             the next step's dispatch order
  learn    evx_replay_sample_blocks   member k's batch into rows [k B, (k + 1) B), one launch
           GroupedLearner.learn_obs   forward pair, TD loss (gamma[k] per row: gamma_row), backward,
                                      clip + Adam with lr[k] (evx_qmlp_adam_pack3_gl): one launch per link

The learner options are opt-in and per member but for Double-Q: n_step[k] > 1 anywhere turns the
sample launch into evx_replay_sample_nstep_blocks (the draws and every member's chain in one launch);
loss[k] = "huber" makes the TD launch evx_td_loss_opt_nets (delta[k] per net, 0 for "mse");
target_tau[k] > 0 anywhere adds one evx_qmlp_polyak_pack3_g launch after the step (members with tau 0
keep their hard copy every target_every[k]); double_q adds one evx_qmlp_act_gb launch on the batch's
s2 blocks for the whole population.

Member k's trajectory, batches and weights are those of a VecTrainer-style loop of its own -- one
``Learner``, one ``Replay``, ``MLPFast.act`` on its row block -- bit for bit (tests/pop_util.py
``SlowPopulation`` is that loop; DESIGN.md 5.5 holds the contract). No host syncs inside ``step()``.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from typing import List, Optional, Sequence

import torch

from ._lib import NSTEP_MAX, OBS_WORDS, check, evx_member_buf, evx_replay, lib
from .env import _check_out_rows, _ptr, _stream

MAX_MEMBERS = 64
_HP = ("lr", "gamma", "epsilon", "epsilon_min", "epsilon_decay", "target_every")
_OPT = ("loss", "huber_delta", "target_tau", "n_step")  # the learner options a member may set for itself


def per_member(name: str, v, K: int) -> list:
    """A hyperparameter as a list of K values: a scalar is broadcast, a sequence must hold K.
    target_every: integers >= 1; epsilon / epsilon_min: finite, in [0, 1]; lr: finite, >= 0;
    gamma / epsilon_decay: finite, in [0, 1]; loss: "mse" or "huber"; huber_delta: finite, > 0;
    target_tau: finite, in [0, 1]; n_step: integers in 1..NSTEP_MAX (32). ValueError naming the value
    otherwise."""
    vals = list(v) if isinstance(v, (list, tuple)) else [v] * K
    if len(vals) != K:
        raise ValueError(f"{name} must be a scalar or a sequence of members = {K} values, not {len(vals)}: {v!r}")
    out = []
    for x in vals:
        if name == "target_every":
            if isinstance(x, bool) or not isinstance(x, int) or x < 1:
                raise ValueError(f"target_every must be an integer >= 1, not {x!r}")
            out.append(x)
            continue
        if name == "n_step":
            if isinstance(x, bool) or not isinstance(x, int) or not 1 <= x <= NSTEP_MAX:
                raise ValueError(f"n_step must be an integer in 1..{NSTEP_MAX}, not {x!r}")
            out.append(x)
            continue
        if name == "loss":
            if x not in ("mse", "huber"):
                raise ValueError(f"loss must be 'mse' or 'huber', not {x!r}")
            out.append(x)
            continue
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
            raise ValueError(f"{name} must be a finite number, not {x!r}")
        if name == "huber_delta":
            if x <= 0:
                raise ValueError(f"huber_delta must be > 0, not {x!r}")
            out.append(float(x))
            continue
        if x < 0 or (name != "lr" and x > 1):
            raise ValueError(f"{name} must lie in " + ("[0, inf)" if name == "lr" else "[0, 1]") + f", not {x!r}")
        out.append(float(x))
    return out


def validate_population(layout, E, members, batch, replay_capacity, learn_every=1, n_step=1) -> int:
    """The constructor's refusals that need no device (ValueError naming the value); returns
    N = (E / members) * R, the rows a member owns. n_step (a scalar or members values): a member's
    ring must hold n_step[k] pushes of N rows, or no chain of its could reach that depth."""
    from .env import LayoutSet
    if isinstance(layout, LayoutSet):
        raise ValueError("PopulationTrainer: one DeviceLayout, not a LayoutSet")
    K = members
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= MAX_MEMBERS:
        raise ValueError(f"members must be an integer in 1..{MAX_MEMBERS}, not {K!r}")
    if isinstance(E, bool) or not isinstance(E, int) or E < K or E % K:
        raise ValueError(f"E must be a positive multiple of members = {K}, not {E!r}")
    N = (E // K) * int(layout.R)
    if N % 2:
        raise ValueError(f"(E / members) * R = {N} must be even (dropout hash rows come in pairs)")
    if isinstance(batch, bool) or not isinstance(batch, int) or batch <= 0 or batch % 2:
        raise ValueError(f"batch must be even and > 0, not {batch!r}")
    C_ = replay_capacity
    if isinstance(C_, bool) or not isinstance(C_, int) or C_ < max(N, batch):
        raise ValueError(f"replay_capacity must hold a member's push of {N} rows and a batch of {batch}, not {C_!r}")
    if isinstance(learn_every, bool) or not isinstance(learn_every, int) or learn_every < 1:
        raise ValueError(f"learn_every must be an integer >= 1, not {learn_every!r}")
    for n in per_member("n_step", n_step, K):
        if n * N > C_:
            raise ValueError(f"n_step = {n} needs a replay_capacity of at least n_step * N = {n * N} slots "
                             f"({n} pushes of {N} rows), not {C_!r}")
    return N


class BlockReplay:
    """K uniform replay rings of one capacity, every array one allocation [K][capacity]
    (evx_replay_push_blocks / evx_replay_sample_blocks); pos and size are common to the rings."""

    def __init__(self, rings: int, capacity: int, device):
        self.K, self.capacity = int(rings), int(capacity)
        n = self.K * self.capacity
        i32 = dict(dtype=torch.int32, device=device)
        self.s = torch.zeros(n * OBS_WORDS, **i32)
        self.s2 = torch.zeros(n * OBS_WORDS, **i32)
        self.a = torch.zeros(n, **i32)
        self.r = torch.zeros(n, dtype=torch.float32, device=device)
        self.done = torch.zeros(n, dtype=torch.uint8, device=device)
        self.c = evx_replay(capacity=self.capacity, s=self.s.data_ptr(), s2=self.s2.data_ptr(), a=self.a.data_ptr(),
                            r=self.r.data_ptr(), done=self.done.data_ptr())
        self.pos = 0
        self.size = 0

    def push(self, s, s2, a, r_env, done_env, n, agents_per_env, s2_term=None):
        """Rows [k n, (k + 1) n) into ring k at pos, every k (s2_term where the row's env is done)."""
        for name, t, per in (("s", s, OBS_WORDS), ("s2", s2, OBS_WORDS), ("s2_term", s2_term, OBS_WORDS), ("a", a, 1)):
            if t is not None and t.numel() < self.K * n * per:
                raise ValueError(f"BlockReplay.push: {name} holds {t.numel() // per} rows, needs {self.K * n}")
        envs = self.K * n // max(1, agents_per_env)
        if r_env.numel() < envs or done_env.numel() < envs:
            raise ValueError(f"BlockReplay.push: r_env / done_env must hold {envs} envs")
        check(lib().evx_replay_push_blocks(C.byref(self.c), s.data_ptr(), s2.data_ptr(), _ptr(s2_term), a.data_ptr(),
                                           r_env.data_ptr(), done_env.data_ptr(), n, self.K, agents_per_env, self.pos,
                                           _stream()), "replay_push_blocks")
        self.pos = (self.pos + n) % self.capacity
        self.size = min(self.capacity, self.size + n)

    def sample(self, B, seed, offset, out):
        """Ring k's B draws under (seed, offset + k B) into rows [k B, (k + 1) B) of out, every k."""
        _check_out_rows("BlockReplay.sample", out, ("s", "s2", "a", "r", "done"), self.K * B, f"needs {self.K * B}")
        check(lib().evx_replay_sample_blocks(C.byref(self.c), self.size, B, self.K, seed, offset, out["s"].data_ptr(),
                                             out["s2"].data_ptr(), out["a"].data_ptr(), out["r"].data_ptr(),
                                             out["done"].data_ptr(), _stream()), "replay_sample_blocks")

    def live_range(self):
        """(base, count) of every ring in push order, oldest first: ((pos - size) mod C, size)."""
        return (self.pos - self.size) % self.capacity, self.size

    def sample_nstep(self, B, seed, offset, n_step, gamma, stride, out):
        """sample()'s draws, each followed by ring k's n-step chain of depth n_step[k] under gamma[k]
        over the live range, stride rows pushed per env step (evx_replay_sample_nstep_blocks, one
        launch): out["s"] / out["a"] the drawn slot's, out["r"] the discounted return, out["s2"] /
        out["done"] the chain's last slot's, out["gamma_row"] = gamma[k]^L; out["nlen"] (int32, L) and
        out["idx"] (int64, the drawn ring-local slot) are optional. Trainer.Replay.sample + .nstep
        of every ring, bit for bit."""
        if len(n_step) != self.K or len(gamma) != self.K:
            raise ValueError(f"BlockReplay.sample_nstep: n_step and gamma must hold {self.K} values")
        _check_out_rows("BlockReplay.sample_nstep", out, ("s", "s2", "a", "r", "done", "gamma_row"), self.K * B,
                       f"needs {self.K * B}", optional=("nlen", "idx"))
        base, count = self.live_range()
        ns = (C.c_int32 * self.K)(*[int(n) for n in n_step])
        gm = (C.c_float * self.K)(*[float(g) for g in gamma])
        check(lib().evx_replay_sample_nstep_blocks(C.byref(self.c), self.size, B, self.K, seed, offset, base, count,
                                                   stride, ns, gm, out["s"].data_ptr(), out["s2"].data_ptr(),
                                                   out["a"].data_ptr(), out["r"].data_ptr(), out["done"].data_ptr(),
                                                   out["gamma_row"].data_ptr(), _ptr(out.get("nlen")),
                                                   _ptr(out.get("idx")), _stream()), "replay_sample_nstep_blocks")


class PopulationTrainer:
    def __init__(self, layout, E: int, members: int, seed_base: int = 1234, seed: int = 0,
                 init_seeds: Optional[Sequence[int]] = None, batch: int = 4096, replay_capacity: int = 1 << 18,
                 lr=1e-4, gamma=0.99, epsilon=1.0, epsilon_min=0.02, epsilon_decay=0.9995, target_every=1000,
                 learn_every: int = 1, episode_stats: bool = False, learn_stats: bool = False,
                 double_q: bool = False, loss="mse", huber_delta=1.0, target_tau=0.0, n_step=1):
        """members = K learners over E envs of one DeviceLayout (E / K each); batch = B rows per member
        and learn step; replay_capacity = C slots per member. lr, gamma, epsilon, epsilon_min,
        epsilon_decay and target_every: a scalar, or a sequence of K values (per_member).
        loss ("mse" / "huber"), huber_delta, target_tau and n_step: the learner options of
        evacx.qnet.Learner and VecTrainer, each a scalar or a sequence of K values (per_member). A
        member with target_tau[k] > 0 blends its target after every learn step and takes no hard copy;
        a member with n_step[k] > 1 learns on returns of up to n_step[k] rewards along its own ring
        (the ring must hold n_step[k] pushes). double_q is one bool for the whole population: the
        selection forward is one launch for all members and LearnStats reads one sel buffer, and it
        fixes the dropout stream numbering (3 per learn step instead of 2), so it cannot change
        later either (per-member Double-Q: not built). With every option at its default nothing
        more is allocated or launched than without them.
        init_seeds[k] (default seed + k): member k starts from Learner(seed=init_seeds[k])'s weights.
        seed keys the dropout hash, the epsilon draws (seed * 7919 + 17) and the replay draws
        (seed * 7919 + 18); env e is seeded seed_base + e. episode_stats / learn_stats: EpisodeStats
        grouped by member / LearnStats(K) for episode_summary() / learn_summary(); off: nothing is
        allocated or launched for them. The net is the x3 MLP; one GPU, strict schedule, uniform
        replay, no act table."""
        N = validate_population(layout, E, members, batch, replay_capacity, learn_every, n_step)
        K = members
        hp = dict(lr=lr, gamma=gamma, epsilon=epsilon, epsilon_min=epsilon_min, epsilon_decay=epsilon_decay,
                  target_every=target_every, loss=loss, huber_delta=huber_delta, target_tau=target_tau, n_step=n_step)
        for name in _HP + _OPT:
            setattr(self, name, per_member(name, hp[name], K))
        if not isinstance(double_q, bool):
            raise ValueError(f"double_q must be a bool (one for the whole population), not {double_q!r}")
        self.double_q = double_q
        if init_seeds is not None and len(init_seeds) != K:
            raise ValueError(f"init_seeds must hold members = {K} seeds, not {len(init_seeds)}")
        from .env import VecEnv
        from .qgroup import GroupedLearner
        self.lay, self.E, self.K, self.R, self.N, self.batch = layout, E, K, layout.R, N, batch
        self.device = layout.device
        self.seed, self.learn_every = int(seed), learn_every
        self.init_seeds = [seed + k for k in range(K)] if init_seeds is None else [int(x) for x in init_seeds]
        self.env = VecEnv(layout, E, obs_buffers=2)  # the push reads env.obs_prev: no copy per step
        self.env.seed([seed_base + i for i in range(E)])
        self.env.reset()
        self.learn_stats = None
        if learn_stats:
            from .lstats import LearnStats
            self.learn_stats = LearnStats(K, self.device)
        self.glearner = GroupedLearner(K, self.device, lr=self.lr[0], gamma=self.gamma[0], seed=self.seed,
                                       init_seeds=self.init_seeds, stats=self.learn_stats)
        self.replay = BlockReplay(K, replay_capacity, self.device)
        dev = self.device
        self.actions = torch.zeros(E * self.R, dtype=torch.int32, device=dev)
        self.samp = dict(s=torch.zeros(K * batch * OBS_WORDS, dtype=torch.int32, device=dev),
                         s2=torch.zeros(K * batch * OBS_WORDS, dtype=torch.int32, device=dev),
                         a=torch.zeros(K * batch, dtype=torch.int32, device=dev),
                         r=torch.zeros(K * batch, dtype=torch.float32, device=dev),
                         done=torch.zeros(K * batch, dtype=torch.uint8, device=dev))
        # gamma[k] on every row of block k (evx_td_opts.gamma_row)
        self.gamma_row = torch.tensor(self.gamma, dtype=torch.float32).repeat_interleave(batch).to(dev)
        self.episodes = None
        if episode_stats:
            from .episodes import EpisodeStats
            self.member_of = torch.arange(K, dtype=torch.int32).repeat_interleave(E // K).to(dev)
            self.episodes = EpisodeStats(E, dev, layout.P, layout_idx=self.member_of, n_layouts=K)
        self.act_seed = self.seed * 7919 + 17
        self.sample_seed = self.seed * 7919 + 18
        self.t = 0
        self.learn_steps = 0
        self.last_loss: Optional[torch.Tensor] = None
        self.env.compute_orders()  # the first step's order (the reset wrote every class byte)

    # ------------------------------------------------------------------ step
    def act(self):
        """One act launch for every member (a fresh dropout stream); returns the actions buffer
        (read it after a synchronize: the kernels run asynchronously)."""
        gl = self.glearner
        gl.drop_stream += 1
        gl.act_blocks(self.lay.c, self.env.obs, self.N, self.epsilon, actions=self.actions, act_seed=self.act_seed,
                      act_offset=self.t * self.E * self.R, drop_stream=gl.drop_stream)
        return self.actions

    def learn(self):
        """One learn step of every member (None while a ring holds fewer than batch rows)."""
        if self.replay.size < self.batch:
            return None
        K, B, sp, gl = self.K, self.batch, self.samp, self.glearner
        grow = self.gamma_row
        if any(n > 1 for n in self.n_step):  # the sampler follows every member's chain in its own launch
            if "gamma_row" not in sp:
                sp.update(gamma_row=torch.zeros(K * B, dtype=torch.float32, device=self.device),
                          nlen=torch.zeros(K * B, dtype=torch.int32, device=self.device))
            self.replay.sample_nstep(B, self.sample_seed, self.learn_steps * K * B, self.n_step, self.gamma, self.N, sp)
            grow = sp["gamma_row"]
        else:
            self.replay.sample(B, self.sample_seed, self.learn_steps * K * B, sp)
        opts = {}
        if self.double_q:
            opts["double_q"] = True
        if any(ls == "huber" for ls in self.loss):  # a member's kernel delta is 0 for "mse"
            opts["huber_delta"] = [d if ls == "huber" else 0.0 for ls, d in zip(self.loss, self.huber_delta)]
        loss = gl.learn_obs(self.lay.c, sp["s"], sp["a"], sp["r"], sp["done"], sp["s2"], B, gamma_row=grow, lr=self.lr,
                            **opts)
        self.learn_steps += 1
        for k in range(K):
            if self.epsilon[k] > self.epsilon_min[k]:  # DQNAgent.learn's schedule (agents/dqn_agent.py:163-164)
                self.epsilon[k] *= self.epsilon_decay[k]
        # a soft member blends after every learn step and takes no hard copy (VecTrainer's target_tau)
        due = [k for k in range(K) if self.target_tau[k] == 0 and self.learn_steps % self.target_every[k] == 0]
        if due:
            gl.sync_target(due)
        if any(t > 0 for t in self.target_tau):
            gl.soft_update(self.target_tau)
        return loss

    @property
    def last_nlen(self):
        """The chain length of every row of the last n-step learn step: int32 [K B] on the device
        (read it after a synchronize); None before the first such step."""
        return self.samp.get("nlen")

    def step(self):
        """One training step of every member on the current stream: act, env.step (auto-reset),
        push, the next step's orders, learn."""
        env = self.env
        self.act()
        env.step(self.actions, order=False, auto_reset=True)
        if self.episodes is not None:
            self.episodes.update(env.reward, env.done, env.counts)
        self.replay.push(env.obs_prev, env.obs, self.actions, env.reward, env.done, self.N, self.R,
                         s2_term=env.obs_term)
        env.compute_orders()
        if self.t % self.learn_every == 0:
            self.last_loss = self.learn()
        self.t += 1

    def sync(self):
        """Wait for the steps so far (they run on the current stream)."""
        torch.cuda.current_stream(self.device).synchronize()

    # ------------------------------------------------------------- summaries
    def episode_summary(self, clear: bool = True) -> dict:
        """EpisodeStats.summary() of the episodes finished since the last clearing call, grouped by
        member: the total's fields, and per_member[k] the same dict of member k's envs."""
        if self.episodes is None:
            raise RuntimeError("episode_summary: the trainer was made with episode_stats=False")
        out = self.episodes.summary(clear=clear)
        out["per_member"] = out.pop("per_layout")
        return out

    def learn_summary(self, clear: bool = True) -> dict:
        """LearnStats.summary() of the learn steps since the last clearing call (per_net[k]: member k)."""
        if self.learn_stats is None:
            raise RuntimeError("learn_summary: the trainer was made with learn_stats=False")
        return self.learn_stats.summary(clear=clear)

    # --------------------------------------------------------------- members
    def _member(self, k) -> int:
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < self.K:
            raise ValueError(f"member must be an integer in 0..{self.K - 1}, not {k!r}")
        return k

    def set_hparams(self, k: int, **hp):
        """Change member k's lr, gamma, epsilon, epsilon_min, epsilon_decay, target_every, loss,
        huber_delta, target_tau or n_step from the next step on (the values are checked as the
        constructor's). double_q is fixed at construction: it fixes the dropout stream numbering."""
        k = self._member(k)
        for name in hp:
            if name not in _HP + _OPT:
                raise ValueError(f"set_hparams: unknown hyperparameter {name!r} (one of {', '.join(_HP + _OPT)})")
        new = {name: per_member(name, v, 1)[0] for name, v in hp.items()}
        if "n_step" in new and new["n_step"] * self.N > self.replay.capacity:
            raise ValueError(f"n_step = {new['n_step']} needs a replay_capacity of at least n_step * N = "
                             f"{new['n_step'] * self.N} slots, not {self.replay.capacity}")
        for name, v in new.items():
            getattr(self, name)[k] = v
        if "gamma" in new:  # (a fill on the current stream, after the learn steps launched so far)
            self.gamma_row[k * self.batch:(k + 1) * self.batch].fill_(new["gamma"])

    def copy_member(self, src: int, dst: int):
        """Member dst takes member src's online and target parameters and Adam moments; dst's operand
        copies of both nets are repacked. Hyperparameters, ring and envs stay dst's own."""
        src, dst = self._member(src), self._member(dst)
        if src == dst:
            return
        gl = self.glearner
        for buf in (gl.flat, gl.tflat, gl.m, gl.v):
            buf[dst].copy_(buf[src])
        gl.fast.nets[dst].repack()
        gl.fast_t.nets[dst].repack()

    def member_map(self, src_map) -> list:
        """src_map as copy_members takes it: K integers in 0..K - 1 whose donors keep their own block
        (src_map[src_map[k]] == src_map[k]). ValueError naming the value otherwise (no device needed)."""
        src = list(src_map) if isinstance(src_map, (list, tuple)) else None
        if src is None or len(src) != self.K:
            raise ValueError(f"src_map must be a sequence of members = {self.K} integers, not {src_map!r}")
        for k, s in enumerate(src):
            if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < self.K:
                raise ValueError(f"src_map[{k}] must be an integer in 0..{self.K - 1}, not {s!r}")
        for k, s in enumerate(src):
            if src[s] != s:
                raise ValueError(f"src_map[{k}] = {s}: member {s} is itself replaced (by {src[s]}); a donor must "
                                 f"keep its own block")
        return src

    def _member_bufs(self):
        """Every [K][...] array a member's learner state lives in, as evx_copy_members takes them:
        flat, tflat, m, v and the nine operand buffers of both nets."""
        gl = self.glearner
        ts = [gl.flat, gl.tflat, gl.m, gl.v] + [fast.bufs[name] for fast in (gl.fast, gl.fast_t) for name in fast.bufs]
        for t in ts:
            assert t.dim() == 2 and t.shape[0] == self.K and t.is_contiguous()
        return (evx_member_buf * len(ts))(*[
            evx_member_buf(base=t.data_ptr(), stride_bytes=t.stride(0) * t.element_size(),
                           bytes=t.shape[1] * t.element_size()) for t in ts])

    def copy_members(self, src_map):
        """copy_member(src_map[k], k) for every member k with src_map[k] != k, in one launch
        (evx_copy_members): the receivers take their donors' online and target parameters, Adam
        moments and the operand copies of both nets -- a pure function of the parameters, so the
        copied operands are the bits a repack would write. src_map: K integers (member_map checks
        them); no donor may itself be replaced. Hyperparameters, ring and envs stay the receiver's
        own. The identity map launches nothing."""
        src = self.member_map(src_map)
        bufs = self._member_bufs()
        check(lib().evx_copy_members(bufs, len(bufs), (C.c_int32 * self.K)(*src), self.K, _stream()), "copy_members")

    def member_learner(self, k: int):
        """An evacx.qnet.Learner holding member k's online and target weights, Adam moments,
        hyperparameters and learner options (a copy: for evacx.evaluate.evaluate and checkpoints)."""
        from .qnet import Learner
        k = self._member(k)
        gl = self.glearner
        tau = self.target_tau[k]
        lr = Learner(kind="mlp", device=self.device, lr=self.lr[k], gamma=self.gamma[k], precision="f32",
                     seed=self.init_seeds[k], double_q=self.double_q, loss=self.loss[k],
                     huber_delta=self.huber_delta[k], target_tau=tau if tau < 1.0 else 0.0)
        lr.target_tau = tau  # (Learner's constructor stops short of 1, the copy every step; its kernel takes it)
        lr.online.flat.copy_(gl.flat[k])
        lr.target.flat.copy_(gl.tflat[k])
        lr.m.copy_(gl.m[k])
        lr.v.copy_(gl.v[k])
        lr.adam_step = gl.adam_step
        lr.weights_written()
        lr.weights_written(target=True)
        return lr

    def checkpoint(self, k: int) -> dict:
        """Member k as the reference's checkpoint dict (agents/dqn_agent.py:174-191: q_network,
        target_network, optimizer, epsilon, steps), plain host tensors and scalars."""
        k = self._member(k)
        gl = self.glearner

        def host(sd):
            return OrderedDict((n, v.detach().cpu().clone()) for n, v in sd.items())
        state = {}
        if gl.adam_step > 0:
            o = 0
            for i, (name, shape) in enumerate(gl.shapes.items()):
                n = int(torch.Size(shape).numel())
                state[i] = {"step": torch.tensor(float(gl.adam_step)),
                            "exp_avg": gl.m[k, o:o + n].view(shape).detach().cpu().clone(),
                            "exp_avg_sq": gl.v[k, o:o + n].view(shape).detach().cpu().clone()}
                o += n
        group = {"lr": self.lr[k], "betas": gl.betas, "eps": gl.eps, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(gl.shapes)))}
        return {"q_network": host(gl.online[k].state_dict()), "target_network": host(gl.target[k].state_dict()),
                "optimizer": {"state": state, "param_groups": [group]}, "epsilon": float(self.epsilon[k]),
                "steps": int(self.learn_steps)}


__all__: List[str] = ["PopulationTrainer", "BlockReplay", "per_member", "validate_population", "MAX_MEMBERS"]
