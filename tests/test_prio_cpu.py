"""Pin the prioritized-replay oracle (oracle/prio_oracle.c).

The reference has no prioritized replay (uniform random.sample over its deque,
Louvre_Evacuation/agents/dqn_agent.py:132), so parity with the reference is not
applicable here: the oracle is pinned by Philox4x32-10's published known-answer
vectors (Random123 kat_vectors), hand-computed segment-tree cases and the sampling
law of proportional prioritization (P(i) = p_i / sum p), and by a reference that is no tree:
with exact leaves the descent must equal a search in the cumulative sum (prio_util). The
entries' argument checks run here too: they return before any device call."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from prio_util import PATTERNS, _u53, check_sample, exact_td, leaf_patterns


def test_philox4x32_10_known_answers():
    kat = [
        ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
        ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
        ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
         [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
    ]
    for ctr, key, want in kat:
        assert list(orc.philox4x32_10(ctr, key)) == want


def test_tree_known_answers():
    C = 1024
    t = orc.PrioTrees(C)
    assert t.max_leaf[0] == 1.0 and t.sum[1] == 0.0 and np.isinf(t.mn[1])
    t.set_range(1022, 4)  # wraps: slots 1022, 1023, 0, 1
    assert t.sum[1] == 4.0 and t.mn[1] == 1.0
    assert [t.sum[C + j] for j in (1022, 1023, 0, 1, 2)] == [1.0, 1.0, 1.0, 1.0, 0.0]
    t.update([1022, 1023, 0, 1], np.array([0.0, 1.0, 2.0, 3.0], np.float32), eps=0.5, alpha=1.0)
    assert t.sum[1] == 8.0 and t.mn[1] == 0.5 and t.max_leaf[0] == 3.5
    # internal nodes are left + right, roots of the halves
    assert t.sum[2] == 2.5 + 3.5 and t.sum[3] == 0.5 + 1.5
    # stratified descent: segment k covers mass [2k, 2k+2); cumulative order is slot 0, 1, ..., 1022, 1023
    seed = 42
    idx, w = t.sample(4, 0.5, seed, 0)
    cum = [(0, 2.5), (1, 6.0), (1022, 6.5), (1023, 8.0)]  # slot, end of its mass interval
    for k in range(4):
        u = (k + _u53(seed, k)) * (8.0 / 4)
        want = next(s for s, end in cum if u < end)
        assert idx[k] == want, (k, u)
        p = t.sum[C + want]
        assert w[k] == np.float32((p / 0.5) ** -0.5)
    # a later duplicate wins (sequential loop)
    t.update([5, 5, 5], np.array([9.0, 1.0, 4.0], np.float32), eps=0.0, alpha=1.0)
    assert t.sum[C + 5] == 4.0 and t.max_leaf[0] == 9.0


def test_hidden_slots_never_sampled_and_new_get_max():
    C = 2048
    t = orc.PrioTrees(C)
    t.set_range(0, 1500)
    rng = np.random.RandomState(1)
    t.update(np.arange(0, 1500, 3), rng.rand(500).astype(np.float32) * 5, eps=1e-6, alpha=0.6)
    t.set_range(1500, 300, 248)  # 300 new at max priority, slots 1800..2047 hidden
    assert np.all(t.sum[C + 1800:] == 0) and np.all(np.isinf(t.mn[C + 1800:]))
    assert np.all(t.sum[C + 1500:C + 1800] == t.max_leaf[0])
    idx, w = t.sample(4096, 0.4, 7, 0)
    assert idx.min() >= 0 and idx.max() < 1800
    assert np.all(w > 0) and np.all(w <= 1.0)
    assert np.all(np.diff(idx) >= 0)  # stratified: segments are in slot order


def test_sampling_law_is_proportional():
    C = 1024
    t = orc.PrioTrees(C)
    t.set_range(0, 64)
    pr = (np.arange(64) % 7 + 1).astype(np.float32)
    t.update(np.arange(64), pr, eps=0.0, alpha=1.0)
    counts = np.zeros(64)
    B = 1 << 14
    for s in range(8):
        idx, _ = t.sample(B, 1.0, 100 + s, 0)
        counts += np.bincount(idx, minlength=C)[:64]
    expect = pr / pr.sum() * counts.sum()
    # stratification makes the counts far tighter than multinomial: within 2 per pass
    assert np.all(np.abs(counts - expect) <= 16 + 1e-9), np.abs(counts - expect).max()


# ------------------------------------------------------------------ a reference that is not a tree
def _exact_tree(C, slots, td):
    """Leaves through the public entry points: everything hidden, then update(eps = 0, alpha = 1)
    with td = m / 1024 (pow(x, 1.0) is exact). -> (tree, leaf vector)."""
    t = orc.PrioTrees(C)
    t.set_range(0, 0, C)
    t.update(slots, td, eps=0.0, alpha=1.0)
    p = np.zeros(C, np.float64)
    p[slots] = td.astype(np.float64)
    assert np.array_equal(t.sum[C:], p) and t.sum[1] == p.sum()
    return t, p


@pytest.mark.parametrize("C", [1024, 2048, 4096])
def test_descent_equals_a_cumulative_sum_search(C):
    """With leaves that are multiples of 2^-10 below 64 every partial sum and every u -= l of the
    descent is exact, so the oracle's tree descent must pick the slots of a plain
    searchsorted(cumsum(p), u): a reference that shares no code and no idea with the tree."""
    rng = np.random.RandomState(C)
    pats = leaf_patterns(C, rng)
    for name in PATTERNS:
        slots = pats[name]
        t, p = _exact_tree(C, slots, exact_td(rng, len(slots)))
        for B in (1, 257, 1000, 4096):
            for beta in (0.0, 0.4, 1.0):
                idx, w = t.sample(B, beta, 11, 3 * B)
                check_sample(p, idx, w, B, beta, 11, 3 * B, what=(C, name, B, beta))
                if beta == 0.0:
                    assert np.all(w == 1.0)


def test_update_ignores_non_finite_priorities():
    """A row whose priority is not finite changes neither its slot's leaf nor max_leaf, but still
    owns its slot when it is the last row naming it (include/evacx.h, evx_prio_update)."""
    C = 1024
    t = orc.PrioTrees(C)
    t.set_range(0, 8)
    t.update(np.arange(8), np.arange(1, 9, dtype=np.float32), eps=0.0, alpha=1.0)  # leaves 1..8, max 8
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    #       slot 0: finite then NaN -> keeps 1     slot 1: NaN then finite -> 0.5
    #       slot 2: +inf only -> keeps 3           slot 3: finite only -> 20 (the new max)
    #       slot 4: finite, +inf, finite -> 0.25   slot 5: NaN, NaN -> keeps 6
    idx = [0, 1, 2, 0, 3, 4, 1, 4, 5, 4, 5]
    td = np.array([9.0, nan, inf, nan, 20.0, 30.0, 0.5, inf, nan, 0.25, nan], np.float32)
    t.update(idx, td, eps=0.0, alpha=1.0)
    assert [t.sum[C + j] for j in range(8)] == [1.0, 0.5, 3.0, 20.0, 0.25, 6.0, 7.0, 8.0]
    assert np.array_equal(t.sum[C:C + 8], t.mn[C:C + 8])
    assert t.max_leaf[0] == 30.0  # every finite row counts for the max, the +inf and NaN rows do not
    assert np.isfinite(t.sum[1:]).all() and t.sum[1] == 1 + 0.5 + 3 + 20 + 0.25 + 6 + 7 + 8 and t.mn[1] == 0.25
    # negative |TD| under a fractional alpha is a NaN priority too
    t.update([6], np.array([-1.0], np.float32), eps=0.0, alpha=0.6)
    assert t.sum[C + 6] == 7.0 and t.max_leaf[0] == 30.0


# ------------------------------------------------------------------ the entries' argument checks
def _fake_tree(C_):
    """An evx_prio over host arrays: the validation returns before any device call, so the
    pointers are never dereferenced."""
    from evacx import _lib
    bufs = dict(sum=np.zeros(8), mn=np.zeros(8), max_leaf=np.zeros(1), owner=np.zeros(8, np.int32))
    return _lib.evx_prio(capacity=C_, **{k: v.ctypes.data for k, v in bufs.items()}), bufs


def test_prio_entries_validate_before_any_launch():
    from evacx import _lib
    L = _lib.lib()
    C_ = 1024
    t, keep = _fake_tree(C_)
    host = dict(s=np.zeros(8, np.int32), s2=np.zeros(8, np.int32), a=np.zeros(8, np.int32),
                r=np.zeros(8, np.float32), done=np.zeros(8, np.uint8))
    ring = _lib.evx_replay(capacity=C_, **{k: v.ctypes.data for k, v in host.items()})
    ring2 = _lib.evx_replay(capacity=2 * C_, **{k: v.ctypes.data for k, v in host.items()})
    idx, td, w = np.zeros(4, np.int64), np.zeros(4, np.float32), np.zeros(4, np.float32)
    outs = [host[k].ctypes.data for k in ("s", "s2", "a", "r", "done")]

    def refused(rc, msg):
        assert rc == -22, msg
        assert msg in L.evx_prio_last_error(), (msg, L.evx_prio_last_error())

    def sample(rp, tree, B, o=outs, i=idx.ctypes.data, ww=w.ctypes.data):
        return L.evx_prio_sample(C.byref(rp), C.byref(tree), B, 0.4, 1, 0, o[0], o[1], o[2], o[3], o[4], i, ww, None)

    for bad in (1000, 512, 1 << 27):  # not a power of two; below 2^10; above 2^26
        tb, kb = _fake_tree(bad)
        rb = _lib.evx_replay(capacity=bad, **{k: v.ctypes.data for k, v in host.items()})
        refused(L.evx_prio_init(C.byref(tb), None), b"capacity must be 2^10..2^26")
        refused(L.evx_prio_set_range(C.byref(tb), 0, 1, 0, None), b"capacity must be 2^10..2^26")
        refused(L.evx_prio_update(C.byref(tb), idx.ctypes.data, td.ctypes.data, 4, 1e-6, 0.6, None),
                b"capacity must be 2^10..2^26")
        refused(sample(rb, tb, 4), b"capacity must be 2^10..2^26")
    refused(L.evx_prio_init(None, None), b"NULL tree")
    # counts
    refused(L.evx_prio_set_range(C.byref(t), 0, -1, 0, None), b"prio_set_range: bad counts")
    refused(L.evx_prio_set_range(C.byref(t), 0, 2, -1, None), b"prio_set_range: bad counts")
    refused(L.evx_prio_set_range(C.byref(t), 0, C_, 1, None), b"prio_set_range: bad counts")
    refused(L.evx_prio_set_range(C.byref(t), 0, 1, C_, None), b"prio_set_range: bad counts")
    # the sampler: capacities, outputs
    refused(sample(ring2, t, 4), b"ring and tree capacities differ")
    refused(L.evx_prio_sample(None, C.byref(t), 4, 0.4, 1, 0, *outs, idx.ctypes.data, w.ctypes.data, None),
            b"ring and tree capacities differ")
    for k in range(5):
        o = list(outs)
        o[k] = None
        refused(sample(ring, t, 4, o=o), b"prio_sample: NULL output")
    # the update: NULL idx / td with rows to read
    refused(L.evx_prio_update(C.byref(t), None, td.ctypes.data, 4, 1e-6, 0.6, None), b"prio_update: NULL argument")
    refused(L.evx_prio_update(C.byref(t), idx.ctypes.data, None, 1, 1e-6, 0.6, None), b"prio_update: NULL argument")
    # nothing to do is not an error, and launches nothing
    assert L.evx_prio_set_range(C.byref(t), 5, 0, 0, None) == 0
    assert L.evx_prio_update(C.byref(t), None, None, 0, 1e-6, 0.6, None) == 0
    assert L.evx_prio_update(C.byref(t), idx.ctypes.data, td.ctypes.data, -3, 1e-6, 0.6, None) == 0
    assert sample(ring, t, 0) == 0 and sample(ring, t, -1, o=[None] * 5) == 0
    del keep
