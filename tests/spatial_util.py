"""The spatial-map update restated in numpy (the rule of include/evacx.h's evx_spatial_update), shared
by the spatial tests; never evacx.spatial's device path itself."""
import numpy as np

SAFE = 1 << 24
DEAD = 1 << 25
MAPS = ("arrive", "stall", "evac", "died", "robot")


def decode(v):
    """(x, y, safe, dead) of pk words."""
    v = np.asarray(v).view(np.uint32).astype(np.int64)
    return v & 0xFFF, (v >> 12) & 0xFFF, (v & SAFE) != 0, (v & DEAD) != 0


class spatial_ref:
    """Host arrays named as the descriptor's; ``update`` is one step of every env."""

    def __init__(self, E, P, R, GX, GY, n_rows=1, layout_idx=None, cap=0):
        self.E, self.P, self.R, self.GX, self.GY, self.n_rows, self.cap = E, P, R, GX, GY, n_rows, cap
        li = np.zeros(E, np.int64) if layout_idx is None else np.asarray(layout_idx, np.int64)
        self.row = np.clip(li, 0, n_rows - 1)
        self.prev = np.zeros((E, P), np.uint32)
        self.n_total = np.zeros(E, np.int64)
        for k in MAPS:
            setattr(self, k, np.zeros((n_rows, GX, GY), np.int64))
        self.steps = np.zeros(n_rows, np.int64)
        self.bad = np.zeros(1, np.int64)

    def _pk(self, pk):
        return np.asarray(pk).view(np.uint32).reshape(self.E, self.P)

    def sync(self, pk, mask=None):
        pk = self._pk(pk)
        on = np.ones(self.E, bool) if mask is None else np.asarray(mask).reshape(self.E) != 0
        self.prev[on] = pk[on]

    def update(self, pk, robots, done):
        pk = self._pk(pk)
        counted = np.ones(self.E, bool) if self.cap <= 0 else self.n_total < self.cap
        ox, oy, osafe, odead = decode(self.prev)
        x, y, safe, dead = decode(pk)
        live = counted[:, None] & ~osafe & ~odead
        out = (x >= self.GX) | (y >= self.GY)
        self.bad[0] += int((live & out).sum())
        live &= ~out
        rows = np.broadcast_to(self.row[:, None], pk.shape)
        moved = x * self.GY + y != ox * self.GY + oy
        classes = dict(evac=safe, died=~safe & dead, arrive=~safe & ~dead & moved, stall=~safe & ~dead & ~moved)
        assert (sum(c.astype(int) for c in classes.values()) == 1).all()  # exactly one class applies
        for name, c in classes.items():
            m = live & c
            np.add.at(getattr(self, name), (rows[m], x[m], y[m]), 1)
        if self.R:
            u = np.asarray(robots).view(np.uint32).reshape(self.E, self.R).astype(np.int64)
            rx, ry = u & 0xFFFF, u >> 16
            on = np.broadcast_to(counted[:, None], u.shape)
            rout = (rx >= self.GX) | (ry >= self.GY)
            self.bad[0] += int((on & rout).sum())
            m = on & ~rout
            np.add.at(self.robot, (np.broadcast_to(self.row[:, None], u.shape)[m], rx[m], ry[m]), 1)
        np.add.at(self.steps, self.row[counted], 1)
        self.prev[:] = pk
        self.n_total += np.asarray(done).reshape(self.E) != 0

    def episodes(self):
        n = np.minimum(self.n_total, self.cap) if self.cap > 0 else self.n_total
        return np.bincount(self.row, weights=n, minlength=self.n_rows).astype(np.int64)

    def arrays(self):
        return {k: getattr(self, k) for k in ("prev", "n_total", *MAPS, "steps", "bad")}


def pack_robots(xy):
    """robots words of [..., 2] positions: (u16)x | (u16)y << 16."""
    xy = np.asarray(xy, np.int64) & 0xFFFF
    return (xy[..., 0] | (xy[..., 1] << 16)).astype(np.uint32).view(np.int32)


def synthetic(P, E=37, R=2, GX=12, GY=9, steps=12, seed=0):
    """A pk sequence with no env behind it: (first pk [E, P], [(pk, robots [E, R], done [E], pk after the
    masked reset)] per step). Persons take random steps on the grid, become safe or dead at random and stay so, a few
    stand outside the grid and so does one robot; where done, the next state is a fresh random one
    (the caller syncs it in, as after a masked reset)."""
    rng = np.random.default_rng(7000 * seed + 31 * P + GX)

    def fresh(n):
        return rng.integers(0, GX, (n, P)), rng.integers(0, GY, (n, P)), np.zeros((n, P), np.int64)
    x, y, fl = fresh(E)

    def word():
        return (x | (y << 12) | (fl << 24)).astype(np.uint32).view(np.int32)
    first, seq = word(), []
    for s in range(steps):
        gone = fl != 0
        move = (rng.random((E, P)) < 0.45) & ~gone
        x = np.where(move, np.clip(x + rng.integers(-1, 2, (E, P)), 0, GX - 1), x)
        y = np.where(move, np.clip(y + rng.integers(-1, 2, (E, P)), 0, GY - 1), y)
        r = rng.random((E, P))
        fl = np.where(gone, fl, np.where(r < 0.06, 1, np.where(r < 0.10, 2, np.where(r < 0.11, 3, 0))))
        if s in (2, 5):  # a few live persons outside the grid, x or y: they come back the step after
            x[s % E, 0], y[(s + 1) % E, P - 1] = GX + 3, GY
            fl[s % E, 0] = fl[(s + 1) % E, P - 1] = 0
        if s in (3, 6):
            x[(s - 1) % E, 0], y[s % E, P - 1] = GX - 1, 0
        rob = np.stack([rng.integers(0, GX, (E, R)), rng.integers(0, GY, (E, R))], -1)
        if s == 4:
            rob[E - 1, R - 1] = (GX, 2)
        done = (rng.random(E) < 0.25).astype(np.uint8)
        done[0] = 0
        seq.append((word(), pack_robots(rob), done))
        n = int(done.sum())
        if n:
            x[done != 0], y[done != 0], fl[done != 0] = fresh(n)
        seq[-1] = seq[-1] + (word(),)  # the state after the masked reset
    return first, seq


def fixture_pk(tr):
    """pk words [records, P] of a trajectory fixture: x | y << 12 | flags << 24 (1 safe, 2 dead)."""
    pos, fl = tr["snap_pos"].astype(np.uint32), tr["snap_flags"].astype(np.uint32)
    return pos[..., 0] | (pos[..., 1] << 12) | (fl << 24)
