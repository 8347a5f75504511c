"""The uniform replay ring without a GPU.

* Every -22 refusal of evx_replay_push, evx_replay_push_term, evx_env_orders_push_sample,
  evx_replay_sample, evx_replay_sample_window and evx_replay_nstep by return code and text (fake
  pointers, nothing launched), and the calls that have nothing to do returning 0 with NULL arrays.
* VecTrainer refuses a ring smaller than one push at construction.
* The sampler's permutation on the CPU restatement (oracle.replay_indices) alone: B = size draws are
  a bijection of the live range at every size from 1 to 1100 and at the sizes around the larger
  Feistel widths, for plain, windowed and per-agent draws; the key's high words matter.
* Draw quality of the algorithm (the device is bit-equal to the restatement, test_replay_gpu.py):
  over 200,000 consecutive offsets under one seed the first draw is uniform over [0, n) and the
  difference of the first two draws uniform over [1, n), by Pearson's chi-square against
  dof + 5 sqrt(2 dof) -- five standard deviations of a chi-square variable, a statistical bound that
  is not tuned to the code. (Below a few dozen entries the pair distribution is far from uniform:
  DESIGN.md states the measured values; trainers never sample a ring smaller than a batch.)"""
import ctypes
import types

import numpy as np
import pytest

from oracle import oracle as orc
from replay_util import RingModel, chi2_bar, chi2_uniform

FAKE = 0x1000  # a non-null address that is never dereferenced


def _m():
    from evacx import _lib
    return _lib


def _err():
    return _m().lib().evx_last_error().decode()


def _ring(cap=512, **kw):
    f = dict(capacity=cap, s=FAKE, s2=FAKE, a=FAKE, r=FAKE, done=FAKE)
    f.update(kw)
    return _m().evx_replay(**f)


RING_FIELDS = ("s", "s2", "a", "r", "done")


# ------------------------------------------------------------------ evx_replay_push / _push_term
def _push(entry, rp=True, ring=None, n=128, apn=4, pos=0, null=None, term=FAKE):
    """(rc, text) of a push; null: which of s, s2, a, r_env, done_env is NULL."""
    m = _m()
    ring = _ring() if ring is None else ring
    ptrs = [FAKE] * 5
    if null is not None:
        ptrs[null] = None
    if entry == "replay_push_term":
        ptrs.insert(2, term)
    rc = getattr(m.lib(), "evx_" + entry)(ctypes.byref(ring) if rp else None, *ptrs, n, apn, pos, None)
    return rc, _err()


@pytest.mark.parametrize("entry", ["replay_push", "replay_push_term"])
def test_push_refusals(entry):
    def refused(text, **kw):
        assert _push(entry, **kw) == (-22, f"{entry}: {text}"), kw
    refused("bad ring (NULL, or capacity < 1)", rp=False)
    refused("bad ring (NULL, or capacity < 1)", ring=_ring(cap=0), n=0)
    refused("bad ring (NULL, or capacity < 1)", ring=_ring(cap=-4))
    for f in RING_FIELDS:
        refused("NULL ring array", ring=_ring(**{f: None}))
    refused("n must be >= 0", n=-4)
    refused("the capacity does not hold n rows", n=516)  # two rows of one push would share a slot
    refused("pos outside [0, capacity)", pos=-1)  # a slot in front of the ring
    refused("pos outside [0, capacity)", pos=512)
    refused("pos outside [0, capacity)", pos=1 << 40)
    refused("n must be a multiple of agents_per_env >= 1", apn=0)  # a division by zero on the device
    refused("n must be a multiple of agents_per_env >= 1", apn=-2)
    refused("n must be a multiple of agents_per_env >= 1", n=126)
    for i in range(5):
        refused("NULL argument", null=i)
    # whatever else is wrong, a push of no rows is still refused for it
    refused("pos outside [0, capacity)", n=0, pos=512)
    refused("n must be a multiple of agents_per_env >= 1", n=0, apn=0)


@pytest.mark.parametrize("entry", ["replay_push", "replay_push_term"])
def test_push_of_nothing_returns_zero(entry):
    m = _m()
    ring = _ring()
    nulls = [None] * (6 if entry == "replay_push_term" else 5)
    assert getattr(m.lib(), "evx_" + entry)(ctypes.byref(ring), *nulls, 0, 4, 511, None) == 0


def test_push_term_takes_a_null_s2_term():
    """s2_term is optional: with n > 0 the call gets past every check (and would launch), so it is
    tried here only where a later check still refuses it."""
    assert _push("replay_push_term", term=None, null=4) == (-22, "replay_push_term: NULL argument")


# ------------------------------------------------------------------ evx_env_orders_push_sample
def _lay(**kw):
    f = dict(L=36, W=30, P=100, R=2, floor=FAKE, cellinfo=FAKE, valid_bits=FAKE, danger_p=FAKE, danger_o=FAKE)
    f.update(kw)
    return _m().evx_layout(**f)


def _fused(lay=True, st=True, state=None, rp=True, ring=None, n=128, apn=2, pos=0, B=0, size=512, null=None,
           out_null=None, outs=True):
    """(rc, text) of evx_env_orders_push_sample over a state of no envs (E = 0: with n = 0 and B = 0
    a valid call has nothing to launch). null: which of s, s2, s2_term, a, r_env, done_env is NULL."""
    m = _m()
    ring = _ring() if ring is None else ring
    state = m.evx_state(E=0, order=FAKE, perm_ws=FAKE) if state is None else state
    ptrs = [FAKE] * 6
    if null is not None:
        ptrs[null] = None
    o = [FAKE if outs else None] * 5
    if out_null is not None:
        o[out_null] = None
    layout = _lay()
    rc = m.lib().evx_env_orders_push_sample(ctypes.byref(layout) if lay else None, ctypes.byref(state) if st else None,
                                            None, ctypes.byref(ring) if rp else None, *ptrs, n, apn, pos, B, size, 7,
                                            0, *o, None)
    return rc, _err()


@pytest.mark.parametrize("B", [0, 64])
def test_fused_push_refusals_do_not_depend_on_B(B):
    """The push's refusals, with and without a batch drawn in the same launch."""
    def refused(text, **kw):
        assert _fused(B=B, **kw) == (-22, text), kw
    refused("layout is NULL", lay=False)
    refused("env_orders_push: state.order / state.perm_ws is NULL", st=False)
    refused("env_orders_push: state.order / state.perm_ws is NULL", state=_m().evx_state(E=0, order=FAKE))
    refused("env_orders_push: replay capacity must be a power of two", rp=False)
    refused("env_orders_push: replay capacity must be a power of two", ring=_ring(cap=0))
    refused("env_orders_push: replay capacity must be a power of two", ring=_ring(cap=96), size=96)
    for f in RING_FIELDS:
        refused("env_orders_push: NULL ring array", ring=_ring(**{f: None}))
    refused("env_orders_push: n must be >= 0", n=-2)
    refused("env_orders_push: the capacity does not hold n rows", n=514)
    refused("env_orders_push: pos outside [0, capacity)", pos=-1)
    refused("env_orders_push: pos outside [0, capacity)", pos=512)
    refused("env_orders_push: n must be a multiple of agents_per_env >= 1", apn=0)
    refused("env_orders_push: n must be a multiple of agents_per_env >= 1", apn=-1)
    refused("env_orders_push: n must be a multiple of agents_per_env >= 1", n=127)
    for i in (0, 1, 3, 4, 5):  # (s2_term, index 2, may be NULL)
        refused("env_orders_push: NULL argument", null=i)


def test_fused_sample_refusals():
    def refused(text, **kw):
        assert _fused(**dict(dict(B=64), **kw)) == (-22, text), kw
    refused("env_orders_push_sample: bad ring size", size=0)
    refused("env_orders_push_sample: bad ring size", size=513)
    refused("env_orders_push_sample: sample larger than population (random.sample)", size=200, B=201)
    for i in range(5):
        refused("env_orders_push_sample: NULL output", out_null=i)


def test_fused_launch_of_nothing_returns_zero():
    """No envs, no rows, no draws: 0 with every array NULL, and nothing launched."""
    assert _fused(n=0, B=0, null=None, outs=False)[0] == 0
    m = _m()
    ring, layout, state = _ring(), _lay(), m.evx_state(E=0, order=FAKE, perm_ws=FAKE)
    rc = m.lib().evx_env_orders_push_sample(ctypes.byref(layout), ctypes.byref(state), None, ctypes.byref(ring),
                                            *[None] * 6, 0, 2, 0, 0, 0, 0, 0, *[None] * 5, None)
    assert rc == 0
    rc = m.lib().evx_env_orders_push(ctypes.byref(layout), ctypes.byref(state), None, ctypes.byref(ring),
                                     *[None] * 6, 0, 2, 0, None)
    assert rc == 0


# ------------------------------------------------------------------ the samplers and the n-step rows
def _sample(entry, rp=True, ring=None, size=512, B=64, null=None, idx=FAKE, base=0):
    m = _m()
    ring = _ring() if ring is None else ring
    ptrs = [FAKE] * 5  # s, s2, a, r, done
    if null is not None:
        ptrs[null] = None
    r = ctypes.byref(ring) if rp else None
    if entry == "replay_sample":
        rc = m.lib().evx_replay_sample(r, size, B, 7, 0, *ptrs, idx, None)
    else:
        rc = m.lib().evx_replay_sample_window(r, base, size, B, 7, 0, *ptrs, idx, None)
    return rc, _err()


@pytest.mark.parametrize("entry", ["replay_sample", "replay_sample_window"])
def test_sample_refusals(entry):
    empty = "replay: empty" if entry == "replay_sample" else "replay: empty window"
    assert _sample(entry, rp=False) == (-22, empty)
    assert _sample(entry, size=0) == (-22, empty)
    for f in RING_FIELDS:
        assert _sample(entry, ring=_ring(**{f: None})) == (-22, f"{entry}: NULL ring array"), f
    for i in range(5):
        assert _sample(entry, null=i) == (-22, f"{entry}: NULL argument"), i
    if entry == "replay_sample":
        assert _sample(entry, size=513) == (-22, "replay: size > capacity")
        assert _sample(entry, size=63) == (-22, "replay: sample larger than population (random.sample)")
    else:
        assert _sample(entry, size=513) == (-22, "replay: bad window")
        assert _sample(entry, base=-1) == (-22, "replay: bad window")
        assert _sample(entry, base=512) == (-22, "replay: bad window")
        assert _sample(entry, size=63) == (-22, "replay: sample larger than the window (random.sample)")
    # nothing to draw: 0 with every output NULL, nothing launched
    m = _m()
    ring = _ring()
    if entry == "replay_sample":
        assert m.lib().evx_replay_sample(ctypes.byref(ring), 512, 0, 7, 0, *[None] * 6, None) == 0
    else:
        assert m.lib().evx_replay_sample_window(ctypes.byref(ring), 3, 512, 0, 7, 0, *[None] * 6, None) == 0


def _nstep(rp=True, ring=None, B=64, null=None):
    m = _m()
    ring = _ring() if ring is None else ring
    ptrs = [FAKE] * 6  # idx | s2, r, done, gamma_row, len
    if null is not None:
        ptrs[null] = None
    rc = m.lib().evx_replay_nstep(ctypes.byref(ring) if rp else None, ptrs[0], B, 0, 512, 128, 3, 0.99, *ptrs[1:],
                                  None)
    return rc, _err()


def test_nstep_null_refusals():
    assert _nstep(rp=False) == (-22, "replay_nstep: bad ring")
    assert _nstep(ring=_ring(cap=0)) == (-22, "replay_nstep: bad ring")
    for i in range(5):  # (len, index 5, may be NULL)
        assert _nstep(null=i) == (-22, "replay_nstep: NULL argument"), i
    for f in ("s2", "r", "done"):  # the arrays the chains read
        assert _nstep(ring=_ring(**{f: None})) == (-22, "replay_nstep: ring without s2 / r / done"), f
    assert _nstep(B=0)[0] == 0


# ------------------------------------------------------------------ VecTrainer's capacity check
def test_vec_trainer_refuses_a_ring_smaller_than_one_push():
    """Raised from the arguments alone, before the layout or a device is touched."""
    from evacx.trainer import VecTrainer
    lay = types.SimpleNamespace(R=4, P=300, device="cpu")
    with pytest.raises(ValueError, match=r"replay_capacity = 255 is smaller than one push of 256 rows"):
        VecTrainer(lay, 64, batch=64, replay_capacity=255)
    with pytest.raises(ValueError, match=r"replay_capacity = 100 is smaller than one push of 128 rows"):
        VecTrainer(lay, 64, batch=64, replay_capacity=100, groups=2)
    # the lagged schedule's window sets a whole step's rows aside, whatever the groups
    with pytest.raises(ValueError, match=r"replay_capacity = 200 is smaller than one push of 256 rows"):
        VecTrainer(lay, 64, batch=64, replay_capacity=200, groups=2, lagged_learn=True)
    with pytest.raises(ValueError, match=r"replay_capacity = 64 is smaller than one push of 256 rows"):
        VecTrainer(lay, 64, batch=64, replay_capacity=64, replay="prioritized")


def test_model_window_and_live_range():
    """The model's own bookkeeping, on the figures test_replay_sample_window_stays_inside uses."""
    ring = RingModel(100)
    z = np.zeros((30, 8), np.int32)
    for _ in range(4):
        ring.push(z, z, np.zeros(30, np.int32), np.zeros(10), np.zeros(10, np.uint8), 30, 3)
    assert (ring.pos, ring.size) == (20, 100)
    assert ring.window(30) == (50, 70) and ring.live_range() == (20, 100)
    ring = RingModel(100)
    ring.push(z, z, np.zeros(30, np.int32), np.zeros(10), np.zeros(10, np.uint8), 30, 3)
    assert ring.window(30) == (0, 30) and ring.live_range() == (0, 30)


# ------------------------------------------------------------------ the permutation property
BIG_SIZES = [4095, 4096, 4097, 65536, 65537, 2 ** 20 + 1]


def test_oracle_draws_are_a_bijection_at_every_size():
    """B = size draws visit every entry once: every size to 1100 (the Feistel width changes after
    4, 16, 64, 256 and 1024) and the sizes around 4^6, 4^8 and 4^10."""
    for size in list(range(1, 1101)) + BIG_SIZES:
        idx = orc.replay_indices(0, size, size, size, 17, 1000 + size)
        assert np.array_equal(np.sort(idx), np.arange(size)), size


@pytest.mark.parametrize("count", [1, 5, 17, 257, 1025])
def test_oracle_window_draws_are_the_window(count):
    cap = 1100
    base = cap - 3  # the window wraps
    idx = orc.replay_indices(base, count, cap, count, 17, 5)
    assert np.array_equal(np.sort(idx), np.sort((base + np.arange(count)) % cap))
    assert np.array_equal((idx - base) % cap, orc.replay_indices(0, count, cap, count, 17, 5))


def test_oracle_streams_and_key_words():
    size, B = 4097, 64
    seed, off = 17, 4096
    keys = [(seed, off, 0), (seed + 2 ** 32, off, 0), (seed, off + 2 ** 32, 0), (seed, off + 1, 0), (seed, off, 1)]
    got = [orc.replay_indices(0, size, size, B, s, o, stream=g) for s, o, g in keys]
    for i in range(len(keys)):
        assert len(np.unique(got[i])) == B
        for j in range(i):
            assert not np.array_equal(got[i], got[j]), (keys[i], keys[j])
    T = 5
    many = orc.replay_indices_offsets(0, size, size, B, seed, off, T)
    for t in range(T):
        assert np.array_equal(many[t], orc.replay_indices(0, size, size, B, seed, off + t))


# ------------------------------------------------------------------ draw quality
QUALITY_T = 200_000


@pytest.mark.parametrize("n", [100, 257, 1000, 4096, 5000])
def test_draw_quality_first_draw_and_first_difference(n):
    idx = orc.replay_indices_offsets(0, n, n, 2, 17, 0, QUALITY_T)
    first = np.bincount(idx[:, 0], minlength=n)
    diff = np.bincount((idx[:, 1] - idx[:, 0]) % n, minlength=n)
    assert len(first) == n and len(diff) == n and diff[0] == 0  # in range, and without replacement
    c_first, c_diff = chi2_uniform(first), chi2_uniform(diff[1:])
    print(f"n = {n}: first draw chi2 {c_first:.0f} (dof {n - 1}, bar {chi2_bar(n - 1):.0f}), "
          f"difference chi2 {c_diff:.0f} (dof {n - 2}, bar {chi2_bar(n - 2):.0f})")
    assert c_first < chi2_bar(n - 1)
    assert c_diff < chi2_bar(n - 2)
