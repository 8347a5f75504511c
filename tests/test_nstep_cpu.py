"""n-step returns from the replay ring without a device: the numpy restatement of
evx_replay_nstep (also the reference of tests/test_nstep_gpu.py) against a naive float64 loop,
the entry's argument checks before any launch, and the runner's flag and config key.

The reference has no n-step target (agents/dqn_agent.py:143-151 is one step deep), so the gather
is pinned by the restatement below: np.float32 scalars in the loop order include/evacx.h states,
a multiply then an add. It is not the code under test."""
import ctypes as C
import math

import numpy as np
import pytest

CAP, STRIDE = 64, 8
# (base, count): part full; full and wrapped; a lagged window
RANGES = [(0, 40), (24, 64), (24, 56)]
NSTEPS = [1, 2, 3, 5]


def np_nstep(r, done, s2, idx, base, count, stride, n_step, gamma):
    """include/evacx.h's per-row loop of evx_replay_nstep. r f32 [C], done u8 [C], s2 i32 [C][8],
    idx int64 [B] -> R f32 [B], gamma_row f32 [B], done u8 [B], s2 i32 [B][8], len i32 [B]."""
    f = np.float32
    cap = len(r)
    assert r.dtype == np.float32 and s2.shape == (cap, 8)
    B = len(idx)
    R, G = np.zeros(B, f), np.zeros(B, f)
    D, S2, L = np.zeros(B, np.uint8), np.zeros((B, 8), np.int32), np.zeros(B, np.int32)
    gam = f(gamma)
    for i in range(B):
        j0 = int(idx[i])
        d0 = (j0 - base) % cap
        j = j0
        acc, g, dn, n = f(r[j0]), gam, int(done[j0]), 1
        while n < n_step and not dn and d0 + n * stride < count:
            j = (j0 + n * stride) % cap
            prod = f(g * f(r[j]))
            acc = f(acc + prod)
            g = f(g * gam)
            dn = int(done[j])
            n += 1
        assert isinstance(acc, np.float32) and isinstance(g, np.float32)
        R[i], G[i], D[i], S2[i], L[i] = acc, g, dn, s2[j], n
    return R, G, D, S2, L


def naive_f64(r, done, idx, base, count, stride, n_step, gamma):
    """The textbook form in Python floats: the slots of the row's own env and robot from its
    position in push order onwards, cut at the first terminal one, at n_step and at the end of
    the range; R = sum_k gamma^k r_k, gamma_row = gamma^len."""
    cap = len(r)
    out_R, out_G = [], []
    for j0 in idx:
        p = (int(j0) - base) % cap
        chain = []
        for q in range(p, max(count, p + 1), stride):
            chain.append((base + q) % cap)
            if done[chain[-1]] or len(chain) == n_step:
                break
        out_R.append(sum(float(gamma) ** k * float(r[j]) for k, j in enumerate(chain)))
        out_G.append(float(gamma) ** len(chain))
    return np.array(out_R, np.float64), np.array(out_G, np.float64)


def ring_fixture(integer_rewards=False, seed=5):
    """The ring of the kernel test (tests/test_nstep_gpu.py): capacity 64, random f32 rewards (or
    small integers, |r| <= 3), done with probability about 0.2, distinct s2 words."""
    rng = np.random.RandomState(seed)
    r = rng.randint(-3, 4, CAP).astype(np.float32) if integer_rewards else (rng.randn(CAP) * 30).astype(np.float32)
    done = (rng.rand(CAP) < 0.2).astype(np.uint8)
    s2 = (np.arange(CAP * 8, dtype=np.int32) * 7 + 100000).reshape(CAP, 8)
    return r, done, s2


def range_slots(base, count):
    return (base + np.arange(count, dtype=np.int64)) % CAP


def test_restatement_matches_a_naive_float64_loop():
    """Integer rewards of magnitude <= 3 and gamma = 0.5: every partial sum is a multiple of
    2^-4 below 8, exact in f32, so the f32 restatement must equal the float64 loop."""
    r, done, s2 = ring_fixture(integer_rewards=True)
    for base, count in RANGES:
        idx = range_slots(base, count)
        for n in NSTEPS:
            R, G, D, S2, L = np_nstep(r, done, s2, idx, base, count, STRIDE, n, 0.5)
            R64, G64 = naive_f64(r, done, idx, base, count, STRIDE, n, 0.5)
            assert np.array_equal(R.astype(np.float64), R64), (base, count, n)
            assert np.array_equal(G.astype(np.float64), G64), (base, count, n)
            assert np.array_equal(G, np.float32(0.5) ** L)
            if n == 1:
                assert np.array_equal(R, r[idx]) and np.array_equal(D, done[idx]) and np.array_equal(S2, s2[idx])
                assert (L == 1).all()


def test_every_stop_cause_occurs_on_the_kernel_fixture():
    """On the fixture the GPU kernel test runs (f32 rewards), for every n_step > 1: chains that
    reach n_step, chains cut by a done, chains cut by the end of the range -- read off len."""
    r, done, s2 = ring_fixture()
    for n in NSTEPS[1:]:
        full = by_done = by_range = 0
        for base, count in RANGES:
            idx = range_slots(base, count)
            _, _, D, S2, L = np_nstep(r, done, s2, idx, base, count, STRIDE, n, 0.99)
            last = (idx + (L - 1).astype(np.int64) * STRIDE) % CAP
            assert np.array_equal(S2, s2[last]) and np.array_equal(D, done[last])
            d0 = (idx - base) % CAP
            full += int(((L == n) & (D == 0)).sum())
            by_done += int(((L < n) & (D != 0)).sum())
            cut = (L < n) & (D == 0)
            assert (d0[cut] + L[cut] * STRIDE >= count).all()  # nothing else ends a chain early
            by_range += int(cut.sum())
        assert full > 0 and by_done > 0 and by_range > 0, (n, full, by_done, by_range)


def test_a_slot_outside_the_range_keeps_its_own_row():
    r, done, s2 = ring_fixture()
    idx = np.array([50, 63, 41], np.int64)  # base 0, count 40: d0 >= count
    R, G, D, S2, L = np_nstep(r, done, s2, idx, 0, 40, STRIDE, 3, 0.99)
    assert (L == 1).all() and np.array_equal(R, r[idx]) and np.array_equal(S2, s2[idx])


# ------------------------------------------------------------------ the entry's argument checks
def _call(L, ring, **kw):
    """evx_replay_nstep with valid host arguments (never dereferenced: validation fails first),
    one of them replaced."""
    bufs = ring["bufs"]
    a = dict(rp=C.byref(ring["c"]), idx=bufs["idx"].ctypes.data, B=4, base=0, count=40, stride=8, n_step=3,
             gamma=0.99, s2=bufs["s2"].ctypes.data, r=bufs["r"].ctypes.data, done=bufs["done"].ctypes.data,
             gamma_row=bufs["g"].ctypes.data, len=None)
    a.update(kw)
    return L.evx_replay_nstep(a["rp"], a["idx"], a["B"], a["base"], a["count"], a["stride"], a["n_step"], a["gamma"],
                              a["s2"], a["r"], a["done"], a["gamma_row"], a["len"], None)


def test_replay_nstep_validates_before_any_launch():
    from evacx import _lib
    L = _lib.lib()
    assert _lib.NSTEP_MAX == 32 and "evx_replay_nstep" in _lib.SIGNATURES
    host = dict(s=np.zeros((CAP, 8), np.int32), s2=np.zeros((CAP, 8), np.int32), a=np.zeros(CAP, np.int32),
                r=np.zeros(CAP, np.float32), done=np.zeros(CAP, np.uint8))
    ring = dict(c=_lib.evx_replay(capacity=CAP, **{k: v.ctypes.data for k, v in host.items()}),
                bufs=dict(idx=np.zeros(4, np.int64), s2=np.zeros((4, 8), np.int32), r=np.zeros(4, np.float32),
                          done=np.zeros(4, np.uint8), g=np.zeros(4, np.float32)))
    bad = [dict(n_step=0), dict(n_step=33), dict(stride=0), dict(count=CAP + 1), dict(count=-1), dict(base=CAP),
           dict(base=-1), dict(idx=None), dict(s2=None), dict(r=None), dict(done=None), dict(gamma_row=None),
           dict(rp=None), dict(gamma=math.nan), dict(gamma=math.inf)]
    for kw in bad:
        rc = _call(L, ring, **kw)
        assert rc == -22, kw
        assert len(L.evx_q_last_error()) > 0, kw
    assert b"n_step" in (_call(L, ring, n_step=33), L.evx_q_last_error())[1]
    assert b"stride" in (_call(L, ring, stride=0), L.evx_q_last_error())[1]
    assert b"NULL" in (_call(L, ring, idx=None), L.evx_q_last_error())[1]
    assert b"gamma" in (_call(L, ring, gamma=math.nan), L.evx_q_last_error())[1]
    # nothing to do is not an error, and launches nothing
    assert _call(L, ring, B=0) == 0


def test_td_opts_mirror_has_the_per_row_discount():
    from evacx.qmlp import evx_td_opts, td_opts
    assert [n for n, _ in evx_td_opts._fields_] == ["sel", "huber_delta", "gamma_row"]
    assert C.sizeof(evx_td_opts) == 24 and evx_td_opts.gamma_row.offset == 16
    o = td_opts()
    assert o.sel is None and o.huber_delta == 0.0 and o.gamma_row is None
    assert td_opts(None, 10.0).gamma_row is None


# ------------------------------------------------------------------ the runner
def test_train_vec_n_step_flag_and_config_key(capsys):
    from Louvre_Evacuation.runners import train_vec as tv
    with pytest.raises(SystemExit) as e:
        tv.parse_args(["--help"])
    assert e.value.code == 0 and "--n-step" in capsys.readouterr().out
    a = tv.parse_args([])
    assert a.n_step is None and tv.n_step_option(a, {}) == 1
    import os
    import yaml
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(tv.__file__), "..", "..", "configs", "dqn.yaml")))
    assert tv.n_step_option(a, cfg["agent"]) == 1      # the reference's agent section has no such key
    assert tv.n_step_option(a, dict(n_step=3)) == 3    # the optional key ...
    assert tv.n_step_option(tv.parse_args(["--n-step", "5"]), dict(n_step=3)) == 5   # ... and the flag over it
    assert tv.n_step_option(tv.parse_args(["--n-step", "1"]), dict(n_step=3)) == 1
    for argv, key in ((["--n-step", "0"], {}), (["--n-step", "33"], {}), ([], dict(n_step=0)), ([], dict(n_step=2.5)),
                      ([], dict(n_step=True))):
        with pytest.raises(ValueError, match="n_step"):
            tv.n_step_option(tv.parse_args(argv), key)
