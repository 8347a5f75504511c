"""Helpers of the population's learner-option tests: ``SlowPopulationOpts`` -- the
contract of PopulationTrainer(double_q, loss, huber_delta, target_tau, n_step) written out with the
single-net pieces only -- and a numpy float32 restatement of evx_replay_sample_nstep_blocks (the
blocked draws, then evx_replay_nstep's chain per ring), which is not the code under test: the draws
come from the oracle's keyed permutation, the chain is include/evacx.h's loop in np.float32 scalars."""
import numpy as np
import torch

import pop_util as pu


class SlowPopulationOpts(pu.SlowPopulation):
    """pop_util.SlowPopulation's loop with the options: K Learner(double_q, loss[k], huber_delta[k],
    target_tau[k]), Replay.sample with out["idx"], Replay.nstep of member k with n_step[k], gamma[k]
    and stride N over its live range, learn_obs(drop_row0=k B, gamma_row), then soft_update() for a
    member with target_tau[k] > 0 and sync_target() every target_every[k] for the others. A Double-Q
    learner advances its dropout stream by 3 per learn step and the population by 3 for all, so
    every learner's drop_stream is set to the population's common value before each call."""

    def __init__(self, layout, E, members, double_q=False, loss="mse", huber_delta=1.0, target_tau=0.0, n_step=1,
                 **kw):
        super().__init__(layout, E, members, **kw)
        from evacx.qnet import Learner
        K, dev = members, layout.device
        self.double_q = double_q
        self.loss_kind, self.huber_delta = pu._list(loss, K), pu._list(huber_delta, K)
        self.target_tau, self.n_step = pu._list(target_tau, K), pu._list(n_step, K)
        seeds = kw.get("init_seeds") or [self.seed + k for k in range(K)]
        self.learners = []
        for k in range(K):
            lr_k = Learner(kind="mlp", device=dev, precision="f32", seed=seeds[k], lr=self.lr[k], gamma=self.gamma[k],
                           double_q=double_q, loss=self.loss_kind[k], huber_delta=self.huber_delta[k],
                           target_tau=self.target_tau[k])
            lr_k.seed = self.seed  # the dropout hash seed is the population's
            self.learners.append(lr_k)
        for sp in self.samp:
            sp.update(idx=torch.zeros(self.batch, dtype=torch.int64, device=dev),
                      gamma_row=torch.zeros(self.batch, dtype=torch.float32, device=dev),
                      nlen=torch.zeros(self.batch, dtype=torch.int32, device=dev))
        self.drop_stream = 0  # the population's

    def step(self):
        K, N, R, B, env = self.K, self.N, self.R, self.batch, self.env
        Ek = self.E // K
        obs = env.obs
        self.drop_stream += 1
        for k, lr in enumerate(self.learners):
            lr.fast.act(self.lay.c, obs[k * N * 8:(k + 1) * N * 8], N, drop=(self.seed, self.drop_stream, 0.2, None, k * N),
                        actions=self.actions[k * N:(k + 1) * N], epsilon=float(self.epsilon[k]),
                        act_seed=self.seed * 7919 + 17, act_offset=self.t * self.E * R + k * N)
        env.step(self.actions, order=False, auto_reset=True)
        for k, rp in enumerate(self.replays):
            rows, envs = slice(k * N * 8, (k + 1) * N * 8), slice(k * Ek, (k + 1) * Ek)
            rp.push(env.obs_prev[rows], env.obs[rows], self.actions[k * N:(k + 1) * N], env.reward[envs], env.done[envs],
                    N, R, s2_term=env.obs_term[rows])
        env.compute_orders()
        if self.t % self.learn_every == 0 and self.replays[0].size >= B:
            nstep_on = any(n > 1 for n in self.n_step)
            for k, (lr, rp, sp) in enumerate(zip(self.learners, self.replays, self.samp)):
                lr.lr, lr.gamma = self.lr[k], self.gamma[k]
                lr.drop_stream = self.drop_stream
                rp.sample(B, self.seed * 7919 + 18, (self.learn_steps * K + k) * B, sp)
                grow = None
                if nstep_on:
                    base, count = rp.live_range()
                    rp.nstep(sp["idx"], B, base, count, N, self.n_step[k], self.gamma[k], sp)
                    grow = sp["gamma_row"]
                lk = lr.learn_obs(self.lay.c, sp["s"], sp["a"], sp["r"], sp["done"], sp["s2"], B, drop_row0=k * B,
                                  gamma_row=grow)
                self.loss[k:k + 1].copy_(lk)
            self.drop_stream += 3 if self.double_q else 2
            self.last_loss = self.loss
            self.learn_steps += 1
            for k, lr in enumerate(self.learners):
                if self.epsilon[k] > self.epsilon_min[k]:
                    self.epsilon[k] *= self.epsilon_decay[k]
                if self.target_tau[k] > 0:
                    lr.soft_update()
                elif self.learn_steps % self.target_every[k] == 0:
                    lr.sync_target()
        self.t += 1


# ------------------------------------------------------------------ the numpy restatement
def np_block_draws(size, B, K, seed, offset):
    """Ring-local slots [K][B] of evx_replay_sample_blocks: ring k draws under (seed, offset + k B)."""
    from oracle import oracle as orc
    return np.stack([np.asarray(orc.replay_indices(0, size, 1 << 40, B, seed, offset + k * B), np.int64)
                     for k in range(K)])


def np_chain(r, done, j0, base, count, stride, n_step, gamma):
    """include/evacx.h's per-row loop on one ring: r f32 [C], done u8 [C], j0 int64 [B] ->
    (R f32, gamma_row f32, done u8, last slot int64, len i32), every product and sum an np.float32."""
    f = np.float32
    cap, B = len(r), len(j0)
    assert r.dtype == np.float32
    R, G = np.zeros(B, f), np.zeros(B, f)
    D, J, L = np.zeros(B, np.uint8), np.zeros(B, np.int64), np.zeros(B, np.int32)
    gam = f(gamma)
    for i in range(B):
        s0 = int(j0[i])
        d0 = (s0 - base) % cap
        j, acc, g, dn, n = s0, f(r[s0]), gam, int(done[s0]), 1
        while n < n_step and not dn and d0 + n * stride < count:
            j = (s0 + n * stride) % cap
            acc = f(acc + f(g * f(r[j])))
            g = f(g * gam)
            dn = int(done[j])
            n += 1
        R[i], G[i], D[i], J[i], L[i] = acc, g, dn, j, n
    return R, G, D, J, L


def np_sample_nstep_blocks(ring, size, pos, B, seed, offset, n_step, gamma, stride):
    """evx_replay_sample_nstep_blocks on host rings: ring = dict(s i32 [K][C][8], s2 i32 [K][C][8], a i32
    [K][C], r f32 [K][C], done u8 [K][C]); the live range ((pos - size) mod C, size). Returns the eight
    outputs as [K][B] arrays: s, s2, a, r, done, gamma_row, len, idx."""
    K, cap = ring["r"].shape
    base, count = (pos - size) % cap, size
    stride = min(stride, cap)
    idx = np_block_draws(size, B, K, seed, offset)
    out = dict(s=np.zeros((K, B, 8), np.int32), s2=np.zeros((K, B, 8), np.int32), a=np.zeros((K, B), np.int32),
               r=np.zeros((K, B), np.float32), done=np.zeros((K, B), np.uint8), gamma_row=np.zeros((K, B), np.float32),
               len=np.zeros((K, B), np.int32), idx=idx)
    for k in range(K):
        R, G, D, J, L = np_chain(ring["r"][k], ring["done"][k], idx[k], base, count, stride, n_step[k], gamma[k])
        out["s"][k], out["a"][k] = ring["s"][k][idx[k]], ring["a"][k][idx[k]]
        out["s2"][k], out["r"][k], out["done"][k], out["gamma_row"][k], out["len"][k] = ring["s2"][k][J], R, D, G, L
    return out


def naive_chain_f64(r, done, j0, base, count, stride, n_step, gamma):
    """The textbook form in Python floats: the slots of the row's own env and robot from its position in
    push order onwards, cut at the first terminal one, at n_step and at the end of the range."""
    cap = len(r)
    Rs, Gs, Ls = [], [], []
    for s0 in j0:
        p = (int(s0) - base) % cap
        chain = []
        for q in range(p, max(count, p + 1), stride):
            chain.append((base + q) % cap)
            if done[chain[-1]] or len(chain) == n_step:
                break
        Rs.append(sum(float(gamma) ** i * float(r[j]) for i, j in enumerate(chain)))
        Gs.append(float(gamma) ** len(chain))
        Ls.append(len(chain))
    return np.array(Rs, np.float64), np.array(Gs, np.float64), np.array(Ls, np.int32)


def stop_causes(L, D, n_step):
    """(chains that reached their member's n_step > 1 without a done, chains cut by a done, chains cut by
    the end of the range) over all members, read off len [K][B] and done [K][B]."""
    full = by_done = by_range = 0
    for k, n in enumerate(n_step):
        Lk, Dk = np.asarray(L[k]), np.asarray(D[k])
        if n > 1:
            full += int(((Lk == n) & (Dk == 0)).sum())
        by_done += int(((Lk < n) & (Dk != 0)).sum())
        by_range += int(((Lk < n) & (Dk == 0)).sum())
    return full, by_done, by_range


# ------------------------------------------------------------------ the sampler test's rings
N_ROWS = 128  # rows per ring and push (the stride of the chains)
NSTEPS, GAMMAS = (1, 3, 32), (0.99, 0.5, 1.0)
# ring state -> pushes of N_ROWS rows. part full: 384 slots (the largest batch, 258, must fit); just full:
# cap 512 after 4 pushes (pos 0), cap 600 after 5 (the fifth straddles the end, pos 40); wrapped: pos 384 / 424
PUSHES = {512: dict(part=3, full=4, wrapped=7), 600: dict(part=3, full=5, wrapped=8)}
# K = 3 takes the three members' (n_step, gamma); K = 1 takes the middle one: with n_step 1 no chain is ever
# cut, and a chain of 32 needs 32 pushes in the range, so neither alone can show the three stop causes
MEMBER_OPTS = {3: (NSTEPS, GAMMAS), 1: (NSTEPS[1:2], GAMMAS[1:2])}


def synthetic_rings(K, cap, pushes, seed=0, exact=False):
    """(ring, size, pos): K host rings after `pushes` pushes of N_ROWS rows. r random f32 (exact: multiples
    of 2^-6 below 4), done with probability 0.1, every s2 word distinct; the slots never pushed hold a
    filler the draws never reach (size counts only pushed slots)."""
    rng = np.random.RandomState(1000 * cap + 10 * pushes + K + seed)
    ring = dict(s=rng.randint(0, 1 << 30, (K, cap, 8)).astype(np.int32),
                s2=(np.arange(K * cap * 8, dtype=np.int32) * 3 + 7).reshape(K, cap, 8),
                a=rng.randint(0, 5, (K, cap)).astype(np.int32),
                r=((rng.randint(-255, 256, (K, cap)) / 64.0) if exact else rng.randn(K, cap) * 30).astype(np.float32),
                done=(rng.rand(K, cap) < 0.1).astype(np.uint8))
    return ring, min(cap, pushes * N_ROWS), (pushes * N_ROWS) % cap
