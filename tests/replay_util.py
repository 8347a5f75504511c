"""A plain model of the uniform replay ring (numpy, no device code) for test_replay_gpu.py and
test_replay_cpu.py.

The ring's contract, as include/evacx.h states it: row i of a push of n rows at pos goes to slot
(pos + i) mod capacity with the team reward (rounded f64 -> f32) and done flag of env
i / agents_per_env, and with s2_term in place of s2 where that env is done; pos advances by n and
size grows to at most capacity. The samplers gather the ring's rows at the slots of a keyed
permutation of the live range; the model takes those slots from oracle.replay_indices (whose own
correctness -- a bijection at every size -- test_replay_cpu.py checks separately) and restates only
which stream and offset each entry uses: stream g for agent g of sample_agents, stream 0 for
sample_joint, offset + k B for ring k of sample_blocks."""
import numpy as np

from oracle import oracle as orc

OBS_WORDS = 8
FIELDS = ("s", "s2", "a", "r", "done")
# what an unwritten slot holds: no push source and no tagged fill produces these
SENTINEL = dict(s=-0x5E5E5E5F, s2=-0x3C3C3C3D, a=-7, r=np.float32(-777.25), done=0xEE)

# rewards the f64 -> f32 rounding must get right: ties between two f32 neighbours (round to even:
# 1 + 2^-24 -> 1, 1 + 3 2^-24 -> 1 + 2^-22), the sign of zero, and values f32 cannot represent
SPECIAL_REWARDS = np.array([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -0.0, 0.1, -1 - 2.0 ** -24, 1e-50, 16777217.0, -0.3])


def _mix(tag, const):
    """[len(tag)][OBS_WORDS] int32 words derived from the tags: another const, other words."""
    t = np.asarray(tag, np.uint64)[:, None]
    w = np.arange(1, OBS_WORDS + 1, dtype=np.uint64)[None, :]
    v = (t * np.uint64(0x9E3779B1) + w * np.uint64(const)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    return v.astype(np.uint32).view(np.int32)


def _coin(tag, salt):
    """A pseudo-random bit per tag."""
    t = (np.asarray(tag, np.uint64) * np.uint64(0x85EBCA6B) + np.uint64(salt)) & np.uint64(0xFFFFFFFF)
    return ((t >> np.uint64(13)) & np.uint64(1)).astype(np.uint8)


def push_rows(n, agents_per_env, tag0, done="mixed"):
    """Sources of one push of n rows, every row recognisable: a[i] = tag0 + i (unique while the tags
    of different pushes do not overlap), s / s2 / s2_term derived from the tag with different
    constants, f64 rewards f32 cannot hold (SPECIAL_REWARDS first), done_env all 0 ("zeros"), all 1
    ("ones") or pseudo-random ("mixed", both values whenever there are two envs)."""
    envs = n // agents_per_env
    a = (tag0 + np.arange(n)).astype(np.int32)
    r_env = (tag0 + np.arange(envs)) * 0.1 + 1.0 / 3.0
    k = min(envs, len(SPECIAL_REWARDS))
    r_env[:k] = SPECIAL_REWARDS[:k]
    if done == "zeros":
        d = np.zeros(envs, np.uint8)
    elif done == "ones":
        d = np.ones(envs, np.uint8)
    else:
        d = _coin(tag0 + np.arange(envs), 17)
        if envs >= 2:
            d[0], d[1] = 0, 1
    return dict(s=_mix(a, 0x01000193), s2=_mix(a, 0x7FEB352D), s2_term=_mix(a, 0x846CA68B), a=a,
                r_env=r_env.astype(np.float64), done_env=d)


class RingModel:
    """One ring. Every slot starts from SENTINEL, so a write a push must not make shows."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.s = np.full((self.capacity, OBS_WORDS), SENTINEL["s"], np.int32)
        self.s2 = np.full((self.capacity, OBS_WORDS), SENTINEL["s2"], np.int32)
        self.a = np.full(self.capacity, SENTINEL["a"], np.int32)
        self.r = np.full(self.capacity, SENTINEL["r"], np.float32)
        self.done = np.full(self.capacity, SENTINEL["done"], np.uint8)
        self.pos = 0
        self.size = 0

    def fill_tagged(self, tag0=1 << 20, slots=None):
        """Older transitions in `slots` (default: every slot): a[slot] = tag0 + slot, s / s2 derived
        from the tag, an f32 reward per tag and a pseudo-random done flag."""
        slots = np.arange(self.capacity) if slots is None else np.asarray(slots)
        tag = tag0 + slots
        self.a[slots] = tag.astype(np.int32)
        self.s[slots] = _mix(tag, 0x2C1B3C6D)
        self.s2[slots] = _mix(tag, 0x297A2D39)
        self.r[slots] = (tag * 0.37 - 11.0).astype(np.float32)
        self.done[slots] = _coin(tag, 5)
        return self

    def push(self, s, s2, a, r_env, done_env, n, agents_per_env, s2_term=None):
        s, s2 = np.asarray(s).reshape(-1, OBS_WORDS), np.asarray(s2).reshape(-1, OBS_WORDS)
        if s2_term is not None:
            s2_term = np.asarray(s2_term).reshape(-1, OBS_WORDS)
        for i in range(n):
            slot = (self.pos + i) % self.capacity
            e = i // agents_per_env
            self.s[slot] = s[i]
            self.s2[slot] = s2_term[i] if s2_term is not None and done_env[e] else s2[i]
            self.a[slot] = a[i]
            self.r[slot] = np.float32(r_env[e])
            self.done[slot] = done_env[e]
        self.pos = (self.pos + n) % self.capacity
        self.size = min(self.capacity, self.size + n)

    def window(self, n_next):
        """(base, count): the newest entries a push of n_next rows does not overwrite."""
        count = min(self.size, self.capacity - n_next)
        return (self.pos - count) % self.capacity, count

    def live_range(self):
        """(base, count) of the whole ring in push order, oldest first."""
        return (self.pos - self.size) % self.capacity, self.size

    def gather(self, idx):
        idx = np.asarray(idx, np.int64)
        out = {k: getattr(self, k)[idx] for k in FIELDS}
        out["idx"] = idx
        return out

    def sample(self, B, seed, offset):
        return self.gather(orc.replay_indices(0, self.size, self.capacity, B, seed, offset))

    def sample_window(self, base, count, B, seed, offset):
        return self.gather(orc.replay_indices(base, count, self.capacity, B, seed, offset))

    def _per_agent(self, B, nets, seed, offset, joint):
        per = self.size // nets  # an agent's population: the slots == agent (mod nets) below size
        idx = [orc.replay_indices(0, per, 1 << 62, B, seed, offset, stream=0 if joint else g) * nets + g
               for g in range(nets)]
        return self.gather(np.concatenate(idx))

    def sample_agents(self, B, nets, seed, offset):
        """Rows [g B, (g + 1) B): agent g's own draws (stream g) among its slots."""
        return self._per_agent(B, nets, seed, offset, joint=False)

    def sample_joint(self, B, nets, seed, offset):
        """Rows [g B, (g + 1) B): agent g's slot of the env-steps stream 0 draws, the same for all."""
        return self._per_agent(B, nets, seed, offset, joint=True)


class BlockModel:
    """K independent rings with a common pos and size (evx_replay_push_blocks / _sample_blocks)."""

    def __init__(self, rings, capacity):
        self.K, self.capacity = rings, capacity
        self.rings = [RingModel(capacity) for _ in range(rings)]

    @property
    def pos(self):
        return self.rings[0].pos

    @property
    def size(self):
        return self.rings[0].size

    def set_pos(self, pos, size):
        for r in self.rings:
            r.pos, r.size = pos, size

    def push_blocks(self, s, s2, a, r_env, done_env, n, agents_per_env, s2_term=None):
        """Rows [k n, (k + 1) n) into ring k; the envs are numbered over all K n rows."""
        s, s2 = np.asarray(s).reshape(-1, OBS_WORDS), np.asarray(s2).reshape(-1, OBS_WORDS)
        if s2_term is not None:
            s2_term = np.asarray(s2_term).reshape(-1, OBS_WORDS)
        epr = n // agents_per_env  # envs per ring (n is a multiple of agents_per_env)
        for k, ring in enumerate(self.rings):
            rows, envs = slice(k * n, (k + 1) * n), slice(k * epr, (k + 1) * epr)
            ring.push(s[rows], s2[rows], a[rows], r_env[envs], done_env[envs], n, agents_per_env,
                      None if s2_term is None else s2_term[rows])

    def sample_blocks(self, B, seed, offset):
        outs = [ring.gather(orc.replay_indices(0, ring.size, ring.capacity, B, seed, offset + k * B))
                for k, ring in enumerate(self.rings)]
        return {f: np.concatenate([o[f] for o in outs]) for f in FIELDS + ("idx",)}

    def stacked(self, field):
        """[K][capacity] as the device holds it."""
        return np.stack([getattr(r, field) for r in self.rings])


def chi2_uniform(counts):
    """Pearson's chi-square of counts against the uniform distribution over len(counts) cells."""
    counts = np.asarray(counts, np.float64)
    exp = counts.sum() / len(counts)
    return float(((counts - exp) ** 2).sum() / exp)


def chi2_bar(dof):
    """dof + 5 sqrt(2 dof): five standard deviations of a chi-square variable above its mean."""
    return dof + 5.0 * np.sqrt(2.0 * dof)
