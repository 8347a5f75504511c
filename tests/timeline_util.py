"""The timeline update restated in numpy (the rule of include/evacx.h's evx_timeline_update), shared
by the timeline tests; never evacx.timeline's device path itself."""
import numpy as np

from golden_util import load

DEAD = 1 << 25
SAFE = 1 << 24
SLOTS = ("evac", "dead", "ended", "seen", "alive", "health_q")


class timeline_ref:
    """Host arrays named as the descriptor's; ``update`` is one step of every env, env by env."""

    def __init__(self, E, P, T, n_rows=1, layout_idx=None, cap=0, track=None):
        self.E, self.P, self.T, self.n_rows, self.cap = E, P, T, n_rows, cap
        self.layout_idx = np.zeros(E, np.int64) if layout_idx is None else np.asarray(layout_idx, np.int64)
        self.t, self.p_evac, self.p_dead = (np.zeros(E, np.int32) for _ in range(3))
        self.n_total = np.zeros(E, np.int64)
        for k in SLOTS:
            setattr(self, k, np.zeros((n_rows, T), np.int64))
        self.late = np.zeros((n_rows, 4), np.int64)
        self.bad_health = np.zeros(1, np.int64)
        self.trk_env, self.trk_person = (np.asarray(v, np.int32) for v in (track or ([], [])))
        n = len(self.trk_env)
        self.trk_pk = np.zeros((T + 1, n), np.uint32)
        self.trk_health = np.zeros((T + 1, n), np.float64)
        self.trk_len = np.zeros(n, np.int32)

    def _trace(self, pk, health, slot0):
        for i, (e, p) in enumerate(zip(self.trk_env, self.trk_person)):
            if self.n_total[e] != 0:
                continue
            slot = 0 if slot0 else int(self.t[e]) + 1
            if slot > self.T:
                continue
            self.trk_pk[slot, i] = pk[e, p]
            self.trk_health[slot, i] = health[e, p]
            self.trk_len[i] = slot + 1

    def trace0(self, pk, health):
        self._trace(np.asarray(pk).view(np.uint32).reshape(self.E, self.P), np.asarray(health).reshape(self.E, self.P),
                    True)

    def update(self, counts, done, pk=None, health=None):
        counts = np.asarray(counts, np.int64).reshape(self.E, 2)
        if pk is not None:
            pk = np.asarray(pk).view(np.uint32).reshape(self.E, self.P)
            health = np.asarray(health, np.float64).reshape(self.E, self.P)
            if len(self.trk_env):
                self._trace(pk, health, False)
        for e in range(self.E):
            k, s, row = int(self.n_total[e]), int(self.t[e]), int(self.layout_idx[e])
            if self.cap <= 0 or k < self.cap:
                d_evac, d_dead = counts[e, 0] - self.p_evac[e], counts[e, 1] - self.p_dead[e]
                if s < self.T:
                    self.evac[row, s] += d_evac
                    self.dead[row, s] += d_dead
                    self.ended[row, s] += int(bool(done[e]))
                    self.seen[row, s] += 1
                    if pk is not None:
                        live = (pk[e] & DEAD) == 0
                        ok = live & (np.abs(health[e]) <= 128)
                        self.alive[row, s] += int(ok.sum())
                        self.health_q[row, s] += int(np.rint(health[e][ok] * 2 ** 20).astype(np.int64).sum())
                        self.bad_health[0] += int((live & ~ok).sum())
                else:
                    self.late[row] += [d_evac, d_dead, int(bool(done[e])), 1]
            if done[e]:
                self.t[e], self.p_evac[e], self.p_dead[e] = 0, 0, 0
                self.n_total[e] = k + 1
            else:
                self.t[e], self.p_evac[e], self.p_dead[e] = s + 1, counts[e, 0], counts[e, 1]

    def arrays(self):
        names = ("t", "p_evac", "p_dead", "n_total", *SLOTS, "late", "bad_health")
        if len(self.trk_env):
            names += ("trk_pk", "trk_health", "trk_len")
        return {k: getattr(self, k) for k in names}


def fixture_pk(tr):
    """pk words [rows, P] of a trajectory fixture: x | y << 12 | flags << 24 (bit 0 safe, bit 1 dead)."""
    pos, fl = tr["snap_pos"].astype(np.uint32), tr["snap_flags"].astype(np.uint32)
    return pos[..., 0] | (pos[..., 1] << 12) | (fl << 24)


_FIX = {}


def fixture(name):
    """(trajectory, pk rows, [(reset row, last row)] per episode), loaded once."""
    if name not in _FIX:
        tr = load(name)
        resets = list(np.nonzero(tr["is_reset"])[0]) + [len(tr["done"])]
        eps = [(int(a), int(b) - 1) for a, b in zip(resets[:-1], resets[1:])]
        assert all(tr["done"][b] and not tr["done"][a:b].any() for a, b in eps)  # rows with is_reset are resets
        _FIX[name] = (tr, fixture_pk(tr), eps)
    return _FIX[name]


def mean_not_dead(flags_row, health_row):
    """get_performance_metrics' avg_health of one recorded step."""
    alive = health_row[(flags_row & 2) == 0]
    return float(np.mean(alive)) if len(alive) else float("nan")
