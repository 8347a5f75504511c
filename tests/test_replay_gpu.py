"""The uniform replay ring on the device against a plain ring model (replay_util.RingModel: a
sequential numpy loop per push, the draws from oracle.replay_indices).

Every comparison is bit for bit over all five arrays of the whole ring (the rewards as their f32
bit patterns, so the sign of zero counts); unwritten slots start from a sentinel, so a stray write
shows.

* evx_replay_push / evx_replay_push_term: rings of 7, 96, 256 and 1000 slots, pushes that wrap, end
  exactly at the ring's end, fill the whole ring (n == capacity) and span three 256-thread blocks;
  done flags all 0, all 1 and mixed; s2_term given and NULL; rewards that tie between two f32
  neighbours; the team reward / done fan-out over 1, 2 and 3 agents per env.
* evx_replay_push_blocks / evx_replay_sample_blocks: 1 and 3 rings against as many model rings.
* evx_env_orders_push_sample, the fused launch, against the model (not against the separate
  launches): draws read from the push's sources and from the ring, on both sides of a wrapping push
  window; the orders against order_util's numpy restatement at env counts around the 64-env wave and
  the 1024-env workgroup, and over VecEnv.split parts, one of whose class bytes are not 16-byte
  aligned (the byte-wise scan).
* The sampler's permutation property: B = size draws of evx_replay_sample are a bijection of
  [0, size) at every size where the Feistel width changes, up to 2^20 + 1; windows that wrap;
  per-agent and joint draws; the key's high words.
Out-of-range calls are tested in test_replay_cpu.py through the host-side refusals only."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from order_util import random_scal, want_order, want_perm
from replay_util import FIELDS, OBS_WORDS, SENTINEL, BlockModel, RingModel, push_rows

pytestmark = pytest.mark.gpu

TAG0 = 1 << 20  # the tagged fill's first tag: a[slot] = TAG0 + slot


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()


def _load(rp, arrays, pos, size):
    """The model's arrays (one ring, or [K][capacity] stacked) onto the device ring."""
    for f in FIELDS:
        getattr(rp, f).copy_(_cuda(arrays(f)))
    rp.pos, rp.size = pos, size


def _device_ring(model):
    from evacx.trainer import Replay
    rp = Replay(model.capacity, "cuda")
    _load(rp, lambda f: getattr(model, f), model.pos, model.size)
    return rp


def _bits(x):
    x = np.ascontiguousarray(x).reshape(-1)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _assert_ring(rp, arrays, what):
    torch.cuda.synchronize()
    for f in FIELDS:
        got, want = getattr(rp, f).cpu().numpy(), arrays(f)
        assert np.array_equal(_bits(got), _bits(want)), (what, f, np.nonzero(_bits(got) != _bits(want))[0][:8])


def _device_rows(rows):
    return {k: _cuda(v) for k, v in rows.items()}


def _out(rows, idx=False):
    """Output buffers of rows + 3 rows, all sentinel: the rows past the batch must stay untouched."""
    n = rows + 3
    out = dict(s=torch.full((n * OBS_WORDS,), SENTINEL["s"], dtype=torch.int32, device="cuda"),
               s2=torch.full((n * OBS_WORDS,), SENTINEL["s2"], dtype=torch.int32, device="cuda"),
               a=torch.full((n,), SENTINEL["a"], dtype=torch.int32, device="cuda"),
               r=torch.full((n,), float(SENTINEL["r"]), dtype=torch.float32, device="cuda"),
               done=torch.full((n,), SENTINEL["done"], dtype=torch.uint8, device="cuda"))
    if idx:
        out["idx"] = torch.full((n,), -9, dtype=torch.int64, device="cuda")
    return out


def _assert_batch(out, want, rows, what):
    """The first `rows` rows of out equal the model's batch; the 3 rows after them are untouched."""
    torch.cuda.synchronize()
    for f in FIELDS + (("idx",) if "idx" in out else ()):
        per = OBS_WORDS if f in ("s", "s2") else 1
        got = out[f].cpu().numpy()
        assert np.array_equal(_bits(got[:rows * per]), _bits(want[f])), (what, f)
        fill = -9 if f == "idx" else SENTINEL[f]
        assert np.all(got[rows * per:] == fill), (what, f, "rows past the batch")


# ------------------------------------------------------------------ evx_replay_push / _push_term
# capacity, first pos, rows per push, agents per env, done pattern of each push
PUSH_CASES = [
    (7, 0, 6, 1, ("ones", "zeros", "mixed")),
    (96, 0, 30, 3, ("mixed", "zeros", "ones", "mixed")),             # the round trip's shape
    (96, 66, 30, 3, ("mixed", "ones", "zeros", "mixed", "mixed")),   # ends exactly at the ring's end, then wraps
    (256, 0, 256, 2, ("mixed", "mixed")),                            # n == capacity, twice
    (1000, 990, 513, 1, ("mixed", "ones")),                          # wraps; two 256-thread blocks plus one row
    (1000, 990, 258, 3, ("mixed", "zeros", "mixed")),
]


@pytest.mark.parametrize("term", [True, False], ids=["s2_term", "no_s2_term"])
@pytest.mark.parametrize("cap,pos0,n,apn,dones", PUSH_CASES, ids=[f"cap{c[0]}-pos{c[1]}-n{c[2]}-apn{c[3]}"
                                                                  for c in PUSH_CASES])
def test_push_matches_model(cap, pos0, n, apn, dones, term):
    _need_gpu()
    model = RingModel(cap)
    if pos0:  # older transitions in front of pos; the slots behind it have never been written
        model.fill_tagged(TAG0, np.arange(pos0))
        model.pos = model.size = pos0
    rp = _device_ring(model)
    for k, done in enumerate(dones):
        rows = push_rows(n, apn, 1000 * (k + 1), done)
        if done == "mixed" and n // apn >= 2:
            assert 0 < rows["done_env"].sum() < n // apn
        d = _device_rows(rows)
        s2_term = rows["s2_term"] if term else None
        model.push(rows["s"], rows["s2"], rows["a"], rows["r_env"], rows["done_env"], n, apn, s2_term)
        rp.push(d["s"], d["s2"], d["a"], d["r_env"], d["done_env"], n, apn, s2_term=d["s2_term"] if term else None)
        _assert_ring(rp, lambda f: getattr(model, f), (k, done))
        assert (rp.pos, rp.size) == (model.pos, model.size), k
        assert rp.window(n) == model.window(n) and rp.live_range() == model.live_range()


def test_push_rounds_rewards_to_nearest_even():
    """What the model's np.float32(r) must give for the rewards every push case carries: the ties go
    to the even neighbour and the sign of zero survives (so a comparison against it means something)."""
    from replay_util import SPECIAL_REWARDS
    r = SPECIAL_REWARDS.astype(np.float32)
    assert r[0] == np.float32(1.0) and r[1] == np.float32(1 + 2.0 ** -22) and np.signbit(r[2]) and r[2] == 0
    assert float(r[3]) != 0.1 and r[4] == np.float32(-1.0) and r[5] == 0 and r[6] == np.float32(16777216.0)


@pytest.mark.parametrize("term", [True, False], ids=["s2_term", "no_s2_term"])
@pytest.mark.parametrize("K,n,pos0", [(1, 6, 90), (3, 6, 90), (1, 30, 66), (3, 30, 66)])
def test_push_blocks_and_sample_blocks_match_model_rings(K, n, pos0, term):
    """K rings of 96 slots: the first push ends exactly at the rings' end, the later ones wrap. Ring
    k's neighbours hold other tags and sentinels, so a row in the wrong ring shows."""
    _need_gpu()
    from evacx.population import BlockReplay
    cap, apn = 96, 3
    model = BlockModel(K, cap)
    for k, ring in enumerate(model.rings):
        ring.fill_tagged(TAG0 * (k + 1), np.arange(pos0))
    model.set_pos(pos0, pos0)
    rp = BlockReplay(K, cap, "cuda")
    _load(rp, model.stacked, pos0, pos0)
    for step, done in enumerate(("mixed", "ones", "zeros", "mixed")):
        rows = push_rows(K * n, apn, 1000 * (step + 1), done)
        d = _device_rows(rows)
        model.push_blocks(rows["s"], rows["s2"], rows["a"], rows["r_env"], rows["done_env"], n, apn,
                          rows["s2_term"] if term else None)
        rp.push(d["s"], d["s2"], d["a"], d["r_env"], d["done_env"], n, apn, s2_term=d["s2_term"] if term else None)
        _assert_ring(rp, model.stacked, (step, done))
        assert (rp.pos, rp.size) == (model.pos, model.size)
        for B in (2, model.size & ~1):  # B == size (even): every ring's batch is a bijection of its slots
            out = _out(K * B)
            rp.sample(B, 21, 1000 + step, out)
            want = model.sample_blocks(B, 21, 1000 + step)
            _assert_batch(out, want, K * B, (step, B))
            if B == model.size:
                for k in range(K):
                    assert np.array_equal(np.sort(want["idx"][k * B:(k + 1) * B]), np.arange(B))


# ------------------------------------------------------------------ evx_env_orders_push_sample
@functools.lru_cache(maxsize=None)
def _layout():
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    return DeviceLayout(build_tables(synthetic(32, 32, 2)), 200)


def _env_with_classes(E, seed):
    """A VecEnv of E envs whose state words are random, its class bytes written from them."""
    from evacx.env import VecEnv
    lay = _layout()
    env = VecEnv(lay, E)
    scal = random_scal(E, int(lay.c.P), int(lay.c.t_max), np.random.default_rng(seed))
    env.scal.view(E, 4).copy_(torch.from_numpy(scal))
    env.refresh_classes()
    return lay, env, scal


def _assert_orders(env, perm, scal, what):
    lay = _layout()
    E = len(scal)
    torch.cuda.synchronize()
    got = perm.cpu().numpy()
    assert np.array_equal(got[:E], want_perm(scal, int(lay.c.t_max))), what
    assert np.all(got[E:] == -7), what
    want, heavy = want_order(scal, int(lay.c.P))
    order = env.order.cpu().numpy()
    assert np.array_equal(order[:E], want), what
    assert order[E] == heavy, what


def _fused(env, scal, cap, pos0, size0, n, B, term=True, seed=77, offset=12345, what=None):
    """One fused launch on a ring of `cap` slots holding size0 tagged entries, against the model's
    push followed by the model's sample. Returns the model's batch."""
    model = RingModel(cap)
    model.fill_tagged(TAG0, np.arange(size0) if size0 < cap else None)
    model.pos, model.size = pos0, size0
    rp = _device_ring(model)
    rows = push_rows(n + 2, 2, 5000, "mixed")  # one env more than the push takes (n == 0: real arrays)
    d = _device_rows(rows)
    E = len(scal)
    perm = torch.full((E + 5,), -7, dtype=torch.int32, device="cuda")
    env.order.fill_(-3)
    out = _out(B)
    model.push(rows["s"], rows["s2"], rows["a"], rows["r_env"], rows["done_env"], n, 2, rows["s2_term"] if term else None)
    rp.push_orders(env, perm, d["s"], d["s2"], d["a"], d["r_env"], d["done_env"], n, 2,
                   s2_term=d["s2_term"] if term else None, sample=(B, seed, offset, out) if B else None)
    _assert_ring(rp, lambda f: getattr(model, f), what)
    assert (rp.pos, rp.size) == (model.pos, model.size), what
    _assert_orders(env, perm, scal, what)
    want = model.sample(B, seed, offset) if B else {f: getattr(model, f)[:0] for f in FIELDS}
    _assert_batch(out, want, B, what)
    return want


def _fused_case(name, cap):
    """(pos0, size0, n, B) in units of capacity / 64."""
    c = cap // 64
    return {"part_old_part_new": (20 * c, 20 * c, 12 * c, 16 * c),   # size < capacity before the first wrap
            "B_eq_size": (20 * c, 20 * c, 12 * c, 32 * c),
            "window_wraps": (58 * c, cap, 12 * c, 40 * c),
            "whole_ring": (10 * c, cap, cap, cap),                   # every draw is read from the push's sources
            "every_slot": (58 * c, cap, 12 * c, cap),                # the slots next to the window's edges included
            "no_batch": (58 * c, cap, 12 * c, 0),
            "no_rows": (20 * c, 20 * c, 0, 16 * c)}[name]


@pytest.mark.parametrize("term", [True, False], ids=["s2_term", "no_s2_term"])
@pytest.mark.parametrize("cap", [64, 1024])
@pytest.mark.parametrize("name", ["part_old_part_new", "B_eq_size", "window_wraps", "whole_ring", "every_slot",
                                  "no_batch", "no_rows"])
def test_fused_launch_matches_model(name, cap, term):
    _need_gpu()
    _, env, scal = _env_with_classes(65, 3)
    pos0, size0, n, B = _fused_case(name, cap)
    want = _fused(env, scal, cap, pos0, size0, n, B, term=term, what=(name, cap))
    idx = want.get("idx", np.zeros(0, np.int64))
    off = (idx - pos0) % cap  # < n: a slot this launch's push wrote
    if name == "part_old_part_new":
        assert np.any(off < n) and np.any(off >= n)
    if name == "B_eq_size":
        assert np.array_equal(np.sort(idx), np.arange(size0 + n))
    if name == "window_wraps":  # drawn slots of the push on both sides of the ring's end, and older ones
        assert np.any((off < n) & (idx >= pos0)) and np.any((off < n) & (idx < pos0)) and np.any(off >= n)
    if name == "whole_ring":
        assert np.array_equal(np.sort(idx), np.arange(cap)) and np.all(off < n)
        assert np.all(want["a"] < TAG0)  # no tagged (older) row survives
    if name == "every_slot":
        assert np.array_equal(np.sort(idx), np.arange(cap)) and np.sum(off < n) == n
    if name == "no_rows":
        assert np.all(want["a"] >= TAG0)


@pytest.mark.parametrize("E", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_fused_launch_orders_at_env_counts(E):
    """The orders of the fused launch around the wave (64 envs) and workgroup (1024 envs) sizes, the
    push wrapping and the batch drawn beside them."""
    _need_gpu()
    _, env, scal = _env_with_classes(E, 100 + E)
    pos0, size0, n, B = _fused_case("window_wraps", 1024)
    _fused(env, scal, 1024, pos0, size0, n, B, what=E)


def test_fused_launch_over_split_parts_unaligned_class_bytes():
    """VecEnv.split parts of 1025 envs each: the second part's class bytes start at byte 1025 of the
    whole env's, which is not 16-byte aligned, so its orders take the byte-wise scan (two order
    workgroups: the second ranks its envs after the first's). The first part's are aligned."""
    _need_gpu()
    _, env, scal = _env_with_classes(2050, 9)
    parts = env.split(2)
    assert parts[0].perm_ws.data_ptr() % 16 == 0 and parts[1].perm_ws.data_ptr() % 16 != 0
    pos0, size0, n, B = _fused_case("window_wraps", 1024)
    for g, part in enumerate(parts):
        _fused(part, scal[g * 1025:(g + 1) * 1025], 1024, pos0, size0, n, B, what=("part", g))


# ------------------------------------------------------------------ the sampler's permutation property
BIG = 2 ** 20 + 1
PERM_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65536, 65537,
              BIG]


@pytest.fixture(scope="module")
def big_ring():
    """One ring of 2^20 + 1 slots with a[slot] = slot, and outputs for as many rows."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from evacx.trainer import Replay
    rp = Replay(BIG, "cuda")
    rp.a.copy_(torch.arange(BIG, dtype=torch.int32, device="cuda"))
    out = dict(s=torch.empty(BIG * OBS_WORDS, dtype=torch.int32, device="cuda"),
               s2=torch.empty(BIG * OBS_WORDS, dtype=torch.int32, device="cuda"),
               a=torch.empty(BIG, dtype=torch.int32, device="cuda"), r=torch.empty(BIG, device="cuda"),
               done=torch.empty(BIG, dtype=torch.uint8, device="cuda"),
               idx=torch.empty(BIG, dtype=torch.int64, device="cuda"))
    return rp, out


def _sample_big(big_ring, size, B, seed, offset):
    from evacx._lib import check, lib
    rp, out = big_ring
    out["a"].fill_(-1)
    out["idx"].fill_(-1)
    check(lib().evx_replay_sample(C.byref(rp.c), size, B, seed, offset, out["s"].data_ptr(), out["s2"].data_ptr(),
                                  out["a"].data_ptr(), out["r"].data_ptr(), out["done"].data_ptr(),
                                  out["idx"].data_ptr(), None), "replay_sample")
    torch.cuda.synchronize()
    return out["idx"][:B].cpu().numpy(), out["a"][:B].cpu().numpy()


@pytest.mark.parametrize("size", PERM_SIZES)
def test_sample_of_the_whole_ring_is_a_bijection(big_ring, size):
    idx, a = _sample_big(big_ring, size, size, 17, 1000 + size)
    assert np.array_equal(np.sort(idx), np.arange(size))
    assert np.array_equal(a, idx)
    assert np.array_equal(idx, orc.replay_indices(0, size, BIG, size, 17, 1000 + size))


def test_sample_key_uses_every_word_of_seed_and_offset(big_ring):
    size, B, seed, off = 4097, 64, 17, 4096
    keys = [(seed, off), (seed + 2 ** 32, off), (seed, off + 2 ** 32), (seed, off + 1)]
    got = []
    for s, o in keys:
        idx, a = _sample_big(big_ring, size, B, s, o)
        assert np.array_equal(idx, orc.replay_indices(0, size, BIG, B, s, o)), (s, o)
        assert np.array_equal(a, idx) and len(np.unique(idx)) == B
        got.append(idx)
    for i in range(len(keys)):
        for j in range(i):
            assert not np.array_equal(got[i], got[j]), (keys[i], keys[j])


@pytest.mark.parametrize("count", [5, 17, 257])
def test_sample_window_that_wraps_is_the_window(count):
    _need_gpu()
    cap = 300
    model = RingModel(cap).fill_tagged(TAG0)
    model.pos, model.size = 0, cap
    rp = _device_ring(model)
    base = cap - 3
    out = _out(count, idx=True)
    rp.sample_window(base, count, count, 9, 70, out)
    want = model.sample_window(base, count, count, 9, 70)
    _assert_batch(out, want, count, count)
    slots = out["a"][:count].cpu().numpy() - TAG0  # the slots, recovered from the gathered tags
    assert np.array_equal(slots, out["idx"][:count].cpu().numpy())
    assert np.array_equal(np.sort(slots), np.sort((base + np.arange(count)) % cap))


@pytest.mark.parametrize("per", [1, 5, 257])
@pytest.mark.parametrize("nets", [1, 2, 8])
def test_per_agent_and_joint_draws(nets, per):
    """B == an agent's whole population: agent g's rows are a bijection of its own slots (== g mod
    nets); the joint rows share one sequence of env-steps; the agents' own sequences differ."""
    _need_gpu()
    from evacx._lib import check, lib
    size = per * nets
    cap = size + 3 * nets  # slots past size are never drawn
    model = RingModel(cap).fill_tagged(TAG0)
    model.pos, model.size = size, size
    rp = _device_ring(model)
    B = per
    steps = {}
    for entry in ("agents", "joint"):
        out = _out(nets * B)
        fn = getattr(lib(), "evx_replay_sample_" + entry)
        check(fn(C.byref(rp.c), size, B, nets, 23, 400, out["s"].data_ptr(), out["s2"].data_ptr(), out["a"].data_ptr(),
                 out["r"].data_ptr(), out["done"].data_ptr(), None), entry)
        want = (model.sample_agents if entry == "agents" else model.sample_joint)(B, nets, 23, 400)
        _assert_batch(out, want, nets * B, entry)
        slots = (out["a"][:nets * B].cpu().numpy() - TAG0).reshape(nets, B)
        for g in range(nets):
            assert np.array_equal(np.sort(slots[g]), np.arange(per) * nets + g), (entry, g)
        steps[entry] = slots // nets
    assert np.all(steps["joint"] == steps["joint"][0])
    if per >= 5:
        seqs = {tuple(row) for row in steps["agents"]}
        assert len(seqs) == nets  # every agent's own permutation (its stream keys it)
        if nets > 1:
            assert tuple(steps["joint"][0]) == tuple(steps["agents"][0])  # the joint draws are stream 0's
