"""Shared helpers of the prioritized-replay tests (tests/test_prio_cpu.py, test_prio_gpu.py,
test_prio_sched_gpu.py): the kernel's 53-bit Philox draw, a cumulative-sum reference of the
stratified sampler that shares nothing with the tree descent, exact leaf patterns, the oracle's
adoption of the device's leaves, and the host shadow of PrioReplay's push / expose."""
import functools

import numpy as np

from oracle import oracle as orc


def _u53(seed, k, offset=0):
    c = k + offset
    q = orc.philox4x32_10([c & 0xFFFFFFFF, c >> 32, 0x9E12A5, 0], [seed & 0xFFFFFFFF, seed >> 32])
    return ((int(q[0]) >> 5) * 67108864.0 + (int(q[1]) >> 6)) / 9007199254740992.0


@functools.lru_cache(maxsize=16)
def u53_array(seed, B, offset=0):
    """U_k for k = 0..B-1 (float64, read-only)."""
    u = np.array([_u53(seed, k, offset) for k in range(B)], np.float64)
    u.setflags(write=False)
    return u


def _adopt_leaves(o, rp):
    """Leaves within 1 ulp, then the oracle takes the GPU's leaves and rebuilds."""
    C = o.C
    gs, gm = rp.tsum.cpu().numpy(), rp.tmin.cpu().numpy()
    ls, lm = gs[C:], gm[C:]
    fin = np.isfinite(o.mn[C:])
    assert np.all(np.abs(ls - o.sum[C:]) <= np.spacing(np.maximum(np.abs(o.sum[C:]), 1e-300)))
    assert np.array_equal(np.isfinite(lm), fin)
    o.sum[C:] = ls
    o.mn[C:] = lm
    o.set_range(0, 0, 0)  # rebuild only
    assert np.array_equal(gs[1:], o.sum[1:]), "sum tree"
    assert np.array_equal(gm[1:], o.mn[1:]), "min tree"
    o.max_leaf[0] = rp.max_leaf.item()


# ------------------------------------------------------------------ exact leaves, plain reference
def exact_td(rng, n):
    """n values m / 1024 as float32, m in [1, 65535]: below 64, multiples of 2^-10. With eps = 0 and
    alpha = 1 they are the leaves themselves, and every partial sum of up to 2^26 of them is an
    integer multiple of 2^-10 below 2^32, exact in float64 in any order of addition."""
    return (rng.randint(1, 65536, size=n).astype(np.float64) / 1024.0).astype(np.float32)


def leaf_patterns(C, rng):
    """name -> sorted live slots (int64): the sweep of the issue."""
    return {
        "all": np.arange(C, dtype=np.int64),
        "random37": np.sort(rng.choice(C, 37, replace=False)).astype(np.int64),
        "slot0": np.array([0], np.int64),
        "last": np.array([C - 1], np.int64),
        # the boundary of two 1024-node blocks (C = 1024 has one block: its two ends)
        "block_edge": np.array([1023, 1024] if C > 1024 else [0, 1023], np.int64),
        "five": np.sort(rng.choice(C, 5, replace=False)).astype(np.int64),  # fewer live leaves than any B > 5
    }


PATTERNS = ("all", "random37", "slot0", "last", "block_edge", "five")


def cumsum_sample(p, B, beta, seed, offset=0):
    """Stratified proportional sampling over the leaf vector p (float64 [C]) without a tree:
    u_k = (k + U_k) * (total / B), idx_k = the slot whose interval of the cumulative sum holds
    u_k. Returns (idx int64 [B], w float64 [B] = (p / p_min)^-beta). Equal to the tree descent
    whenever the cumulative sums are exact (exact_td)."""
    p = np.asarray(p, np.float64)
    cum = np.cumsum(p)
    total = cum[-1]
    u = (np.arange(B, dtype=np.float64) + u53_array(seed, B, offset)) * (total / float(B))
    idx = np.searchsorted(cum, u, side="right").astype(np.int64)
    assert idx.max() < len(p), "a draw at or past the total mass"
    w = (p[idx] / p[p > 0].min()) ** -float(beta)
    return idx, w


def check_sample(p, idx, w, B, beta, seed, offset=0, what=""):
    """idx (int64 [B]) and w (float32 [B]) of a sampler over the exact leaves p against the
    cumulative-sum reference: indices exact, weights within 1 float32 ulp of the float64 value,
    every slot's count within [floor(x) - 1, ceil(x) + 1] of its stratification bound
    x = p_i B / total, and no sampled slot with a zero leaf."""
    ri, rw = cumsum_sample(p, B, beta, seed, offset)
    assert np.array_equal(np.asarray(idx), ri), (what, "indices")
    w = np.asarray(w)
    assert w.dtype == np.float32
    assert np.all(np.abs(w.astype(np.float64) - rw) <= np.spacing(rw.astype(np.float32)).astype(np.float64)), \
        (what, "weights")
    assert np.all(p[idx] > 0), (what, "a sampled slot with a zero leaf")
    x = p * (B / p.sum())
    cnt = np.bincount(idx, minlength=len(p))
    assert np.all(cnt >= np.floor(x) - 1) and np.all(cnt <= np.ceil(x) + 1), (what, "stratification bound")


# ------------------------------------------------------------------ the host shadow of PrioReplay
class ShadowPrio:
    """PrioReplay's host bookkeeping (pos, size, unexposed) over an oracle tree: push() and
    expose() restate evacx/prio.py, window() restates Replay.window."""

    def __init__(self, capacity):
        self.C = int(capacity)
        self.o = orc.PrioTrees(self.C)
        self.pos = self.size = self.unexposed = 0

    def push(self, n):
        """-> the slots written."""
        slots = (self.pos + np.arange(n, dtype=np.int64)) % self.C
        self.pos = (self.pos + n) % self.C
        self.size = min(self.C, self.size + n)
        self.unexposed = min(self.C, self.unexposed + n)
        return slots

    def expose(self, n_hide=0):
        """-> the slots that took the max priority."""
        n_new = min(self.unexposed, self.C - n_hide)
        start = (self.pos - n_new) % self.C
        self.o.set_range(start, n_new, n_hide)
        self.unexposed = 0
        return (start + np.arange(n_new, dtype=np.int64)) % self.C

    def window(self, n_next):
        count = min(self.size, self.C - n_next)
        return (self.pos - count) % self.C, count
