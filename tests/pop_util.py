"""Helpers of the population tests: the shared small env, and ``SlowPopulation`` -- the contract of
evacx.population.PopulationTrainer written out with the single-net pieces only:
one VecEnv, K ``Learner``s, K ``Replay``s and K ``MLPFast.act`` calls on the members' row blocks."""
import functools

import torch

OPERANDS = ("w1b", "w1l", "b1c", "w2b", "w2l", "w2t", "w2tl", "w1o", "w1ol")  # MLPFast.buffer_sizes(x3)
GRID, PEOPLE, R = 48, 300, 4  # the shape of tests/test_qgroup_gpu.py's _env_obs


@functools.lru_cache(maxsize=None)
def small_layout():
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    return DeviceLayout(build_tables(synthetic(GRID, GRID, R)), PEOPLE)


@functools.lru_cache(maxsize=None)
def small_env(E=160, steps=5):
    """(layout, env): E envs of the small layout after a few random steps (read-only for the tests)."""
    from evacx.env import VecEnv
    lay = small_layout()
    env = VecEnv(lay, E)
    env.seed([91 + i for i in range(E)])
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(steps):
        env.step(torch.randint(0, 5, (E * R,), device="cuda", dtype=torch.int32, generator=g))
    torch.cuda.synchronize()
    return lay, env


def _list(v, K):
    return list(v) if isinstance(v, (list, tuple)) else [v] * K


class SlowPopulation:
    """PopulationTrainer's step, member by member. Member k owns envs [k E/K, (k + 1) E/K), rows
    [k N, (k + 1) N): its Learner (initial weights of seed init_seeds[k], the population's dropout
    seed, its own lr and gamma), its Replay, its epsilon schedule and target period."""

    def __init__(self, layout, E, members, seed_base=1234, seed=0, init_seeds=None, batch=256, replay_capacity=1024,
                 lr=1e-4, gamma=0.99, epsilon=1.0, epsilon_min=0.02, epsilon_decay=0.9995, target_every=1000,
                 learn_every=1):
        from evacx.env import VecEnv
        from evacx.qnet import Learner
        from evacx.trainer import Replay
        K = members
        self.lay, self.E, self.K, self.R, self.batch = layout, E, K, layout.R, batch
        self.N = (E // K) * layout.R
        self.seed, self.learn_every = seed, learn_every
        self.lr, self.gamma = _list(lr, K), _list(gamma, K)
        self.epsilon, self.epsilon_min = _list(epsilon, K), _list(epsilon_min, K)
        self.epsilon_decay, self.target_every = _list(epsilon_decay, K), _list(target_every, K)
        seeds = [seed + k for k in range(K)] if init_seeds is None else list(init_seeds)
        self.env = VecEnv(layout, E, obs_buffers=2)
        self.env.seed([seed_base + i for i in range(E)])
        self.env.reset()
        dev = layout.device
        self.learners = []
        for k in range(K):
            lr_k = Learner(kind="mlp", device=dev, precision="f32", seed=seeds[k], lr=self.lr[k], gamma=self.gamma[k])
            lr_k.seed = seed  # the dropout hash seed is the population's
            self.learners.append(lr_k)
        self.replays = [Replay(replay_capacity, dev) for _ in range(K)]
        self.samp = [dict(s=torch.zeros(batch * 8, dtype=torch.int32, device=dev),
                          s2=torch.zeros(batch * 8, dtype=torch.int32, device=dev),
                          a=torch.zeros(batch, dtype=torch.int32, device=dev),
                          r=torch.zeros(batch, dtype=torch.float32, device=dev),
                          done=torch.zeros(batch, dtype=torch.uint8, device=dev)) for _ in range(K)]
        self.actions = torch.zeros(E * self.R, dtype=torch.int32, device=dev)
        self.loss = torch.zeros(K, dtype=torch.float32, device=dev)
        self.t = self.learn_steps = 0
        self.last_loss = None

    def step(self):
        K, N, R, B, env = self.K, self.N, self.R, self.batch, self.env
        Ek = self.E // K
        obs = env.obs
        for k, lr in enumerate(self.learners):
            lr.drop_stream += 1
            lr.fast.act(self.lay.c, obs[k * N * 8:(k + 1) * N * 8], N, drop=(self.seed, lr.drop_stream, 0.2, None, k * N),
                        actions=self.actions[k * N:(k + 1) * N], epsilon=float(self.epsilon[k]),
                        act_seed=self.seed * 7919 + 17, act_offset=self.t * self.E * R + k * N)
        env.step(self.actions, order=False, auto_reset=True)
        for k, rp in enumerate(self.replays):
            rows, envs = slice(k * N * 8, (k + 1) * N * 8), slice(k * Ek, (k + 1) * Ek)
            rp.push(env.obs_prev[rows], env.obs[rows], self.actions[k * N:(k + 1) * N], env.reward[envs], env.done[envs],
                    N, R, s2_term=env.obs_term[rows])
        env.compute_orders()
        if self.t % self.learn_every == 0 and self.replays[0].size >= B:
            for k, (lr, rp, sp) in enumerate(zip(self.learners, self.replays, self.samp)):
                lr.lr, lr.gamma = self.lr[k], self.gamma[k]
                rp.sample(B, self.seed * 7919 + 18, (self.learn_steps * K + k) * B, sp)
                lk = lr.learn_obs(self.lay.c, sp["s"], sp["a"], sp["r"], sp["done"], sp["s2"], B, drop_row0=k * B)
                self.loss[k:k + 1].copy_(lk)
            self.last_loss = self.loss
            self.learn_steps += 1
            for k, lr in enumerate(self.learners):
                if self.epsilon[k] > self.epsilon_min[k]:
                    self.epsilon[k] *= self.epsilon_decay[k]
                if self.learn_steps % self.target_every[k] == 0:
                    lr.sync_target()
        self.t += 1
