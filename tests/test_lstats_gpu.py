"""Learner diagnostics on the GPU (csrc/lstats.hip: evx_lstats_*, evx_vprobe_*; evacx.lstats;
Learner / GroupedLearner / VecTrainer / train_vec wiring).

The reference has none of it, so the kernels are held to the numpy restatements of
tests/lstats_util.py (pinned by tests/test_lstats_cpu.py) bit for bit: every per-row float32 value,
every integer count, and every float64 sum in the order include/evacx.h states. The wiring is held
to "only reads": a learner or trainer with the diagnostics on leaves the same bits as one without."""
import csv
import ctypes as C

import numpy as np
import pytest
import torch

import lstats_util as lu

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
CANARY = 16  # elements behind every array


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _sync():
    torch.cuda.synchronize()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_f64(a, b):
    return np.array_equal(lu.bits(a), lu.bits(b))


# ------------------------------------------------------------------ 1. evx_lstats_update
class _Window:
    """An evx_lstats over arrays with CANARY sentinel elements behind each (and so behind the last net)."""

    def __init__(self, nets, A):
        from evacx import _lib
        self.nets, self.A = nets, A
        self.c = _lib.evx_lstats(nets=nets, A=A)
        self.t, self.n = {}, {}
        for name in lu.I64 + ("act_hist", "td_hist"):
            per = {"act_hist": lu.MAX_A, "td_hist": lu.TD_BUCKETS}.get(name, 1)
            self._make(name, nets * per, torch.int64, -77)
        for name in lu.SUMS + lu.EXT:
            self._make(name, nets, torch.float64, 1234.5)

    def _make(self, name, n, dtype, fill):
        t = torch.full((n + CANARY,), fill, dtype=dtype, device=DEV)
        self.t[name], self.n[name] = t, n
        setattr(self.c, name, t.data_ptr())

    def host(self, g):
        """Net g's fields as lstats_util's window dict; asserts every canary."""
        w = {}
        for name, t in self.t.items():
            h, n = t.cpu().numpy(), self.n[name]
            fill = -77 if h.dtype == np.int64 else 1234.5
            assert (h[n:] == fill).all(), f"canary behind {name}"
            per = n // self.nets
            w[name] = h[g * per:(g + 1) * per].copy() if per > 1 else h[g]
        return w


def _inputs(B, nets, A, seed):
    """nets * B rows: Q / Qt of the project's 1e4 magnitude with ties, actions and sel beyond 0..A-1,
    mixed done, row discounts, and planted NaN / +-inf in Q, Qt and rew."""
    rng = np.random.RandomState(seed)
    n = nets * B
    Q = (rng.randn(n, A) * 2e4).astype(F32)
    Qt = (rng.randn(n, A) * 2e4).astype(F32)
    tie = rng.rand(n) < 0.3
    Q[tie, A - 1] = Q[tie].max(axis=1)  # a later column ties the maximum: the first one counts
    Qt[tie, 0] = Qt[tie].max(axis=1)
    Q[rng.rand(n) < 0.05] = F32(3.5)  # whole rows equal
    act = rng.randint(-1, A + 1, size=n).astype(np.int32)
    greedy = rng.rand(n) < 0.4
    act[greedy] = lu.first_max(Q)[1][greedy]
    rew = (rng.randn(n) * 300).astype(F32)
    done = (rng.rand(n) < 0.3).astype(np.uint8) * rng.randint(1, 256, size=n).astype(np.uint8)
    sel = rng.randint(-2, A + 2, size=n).astype(np.int32)
    grow = (0.99 ** rng.randint(1, 6, size=n)).astype(F32)
    if n >= 2:  # row 1 of the smallest case; a handful of each kind in the larger ones
        k = max(1, n // 60)
        for arr, val in ((Q, np.nan), (Q, np.inf), (Qt, -np.inf), (Qt, np.nan), (rew, np.inf), (rew, -np.inf)):
            idx = rng.choice(np.arange(1, n), size=k, replace=False)
            if arr.ndim == 2:
                arr[idx, rng.randint(0, A, size=k)] = val
            else:
                arr[idx] = val
    return dict(Q=Q, Qt=Qt, act=act, rew=rew, done=done, sel=sel, grow=grow)


def _run_update(win, d, B, gamma, use_sel, use_grow, loss, norm, max_norm, dout, ws):
    from evacx import _lib
    o = _lib.evx_td_opts(sel=d["sel"].data_ptr() if use_sel else None, huber_delta=123.0,
                         gamma_row=d["grow"].data_ptr() if use_grow else None)
    _lib.check(_lib.lib().evx_lstats_update(
        C.byref(win.c), d["Q"].data_ptr(), d["Qt"].data_ptr(), d["act"].data_ptr(), d["rew"].data_ptr(),
        d["done"].data_ptr(), gamma, B, C.byref(o) if (use_sel or use_grow) else None,
        None if loss is None else loss.data_ptr(), None if norm is None else norm.data_ptr(), max_norm,
        None if dout is None else dout.data_ptr(), ws.data_ptr(), ws.numel() - CANARY, None), "lstats_update")


def _check_window(win, want, what):
    for g, w in enumerate(want):
        got = win.host(g)
        for k in lu.I64:
            assert int(got[k]) == int(w[k]), (what, g, k, int(got[k]), int(w[k]))
        for k in ("act_hist", "td_hist"):
            assert np.array_equal(got[k], w[k]), (what, g, k, got[k], w[k])
        for k in lu.SUMS + lu.EXT:
            assert _same_f64(got[k], w[k]), (what, g, k, float(got[k]), float(w[k]))


LSTATS_CASES = [(2, 1, 5), (255, 1, 5), (256, 1, 5), (257, 3, 5), (513, 2, 5), (4098, 1, 5), (257, 2, 3)]


@pytest.mark.parametrize("B,nets,A", LSTATS_CASES)
def test_lstats_update_matches_the_restatement_bit_for_bit(B, nets, A):
    _need_gpu()
    from evacx import _lib
    L = _lib.lib()
    gamma = 0.99
    win = _Window(nets, A)
    need = int(L.evx_lstats_ws_doubles(B, nets))
    assert need == nets * ((B + 255) // 256) * 10
    ws = torch.full((need + CANARY,), 4321.0, dtype=torch.float64, device=DEV)
    _lib.check(L.evx_lstats_init(C.byref(win.c), None), "lstats_init")
    want = [lu.empty_window() for _ in range(nets)]
    _check_window(win, want, "empty")
    host = [_inputs(B, nets, A, seed=1000 * B + nets + s) for s in range(4)]
    dev = [{k: _dev(v) for k, v in h.items()} for h in host]
    # four consecutive updates accumulate: plain, sel, gamma_row, both; loss / norm given, absent, not finite
    steps = [(False, False, 3.0e4, 0.5, 1.0), (True, False, None, 2.5, 1.0), (False, True, np.nan, 0.25, 1.0),
             (True, True, 7.0, 1.5, 0.0)]
    snaps = []
    for (use_sel, use_grow, loss, norm, max_norm), h, d in zip(steps, host, dev):
        lv = None if loss is None else _dev(np.full(nets, loss, F32) + np.arange(nets, dtype=F32))
        nv = _dev(np.full(nets, norm, F32) + np.arange(nets, dtype=F32))
        dout = torch.full((nets * B + CANARY,), 7.0, dtype=torch.float32, device=DEV)
        _run_update(win, d, B, gamma, use_sel, use_grow, lv, nv, max_norm, dout, ws)
        _sync()
        got_d = dout.cpu().numpy()
        assert (got_d[nets * B:] == 7.0).all() and (ws[need:].cpu().numpy() == 4321.0).all(), "canary"
        for g in range(nets):
            s = slice(g * B, (g + 1) * B)
            ref_d = lu.fold(want[g], h["Q"][s], h["Qt"][s], h["act"][s], h["rew"][s], h["done"][s], F32(gamma),
                            sel=h["sel"][s] if use_sel else None, gamma_row=h["grow"][s] if use_grow else None,
                            loss=None if loss is None else F32(loss) + F32(g), norm=F32(norm) + F32(g),
                            max_norm=max_norm)
            assert np.array_equal(np.isnan(got_d[s]), np.isnan(ref_d)), ("d_out NaN rows", g)
            ok = ~np.isnan(ref_d)
            assert np.array_equal(got_d[s][ok].view(np.uint32), ref_d[ok].view(np.uint32)), ("d_out", g)
        _check_window(win, want, f"after update {len(snaps)}")
        snaps.append({k: t.clone() for k, t in win.t.items()})
    assert all(int(w["rows_bad"]) > 0 for w in want) and all(int(w["steps_bad"]) == 1 for w in want)
    assert all(int(w["rows"]) == 4 * B for w in want)
    # init empties the window; the same four updates give the same bits again
    _lib.check(L.evx_lstats_init(C.byref(win.c), None), "lstats_init")
    _sync()
    _check_window(win, [lu.empty_window() for _ in range(nets)], "after init")
    for i, ((use_sel, use_grow, loss, norm, max_norm), d) in enumerate(zip(steps, dev)):
        lv = None if loss is None else _dev(np.full(nets, loss, F32) + np.arange(nets, dtype=F32))
        nv = _dev(np.full(nets, norm, F32) + np.arange(nets, dtype=F32))
        _run_update(win, d, B, gamma, use_sel, use_grow, lv, nv, max_norm, None, ws)
        _sync()
        for k, t in win.t.items():
            a, b = t.view(torch.int64), snaps[i][k].view(torch.int64)
            assert torch.equal(a, b), ("second run", i, k)
    if nets > 1:  # another net's inputs do not reach net g
        other = {k: v.clone() for k, v in dev[0].items()}
        for k in ("Q", "Qt", "rew"):
            other[k][:B] = other[k][:B] * 0.5 + 1.0
        other["act"][:B] = 0
        other["done"][:B] = 1
        _lib.check(L.evx_lstats_init(C.byref(win.c), None), "lstats_init")
        _run_update(win, other, B, gamma, False, False, None, None, 0.0, None, ws)
        _sync()
        moved = [lu.empty_window() for _ in range(nets)]
        for g in range(1, nets):
            s = slice(g * B, (g + 1) * B)
            h = host[0]
            lu.fold(moved[g], h["Q"][s], h["Qt"][s], h["act"][s], h["rew"][s], h["done"][s], F32(gamma))
            got = win.host(g)
            for k in lu.I64:
                assert int(got[k]) == int(moved[g][k]), (g, k)
            for k in lu.SUMS + lu.EXT:
                assert _same_f64(got[k], moved[g][k]), (g, k)
            assert np.array_equal(got["td_hist"], moved[g]["td_hist"])


# ------------------------------------------------------------------ 2. the learner
def _env_obs(E=160, R=4, steps=7, grid=48, people=300):
    from evacx.env import DeviceLayout, VecEnv
    from evacx.layout import build_tables, synthetic
    lay = DeviceLayout(build_tables(synthetic(grid, grid, R)), people)
    env = VecEnv(lay, E)
    env.seed([77 + i for i in range(E)])
    env.reset()
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(steps):
        env.step(torch.randint(0, 5, (E * R,), device=DEV, dtype=torch.int32, generator=g))
    _sync()
    return lay, env


@pytest.fixture(scope="module")
def small_env():
    _need_gpu()
    return _env_obs()


def _batch(env, lay, n, g):
    """n rows of s and s' from the env's observations, actions, rewards randn * 300 and 20 % done flags."""
    perm = torch.randperm(env.E * lay.R, generator=g)
    obs = env.obs.view(-1, 8)
    s_obs = obs[perm[:n].to(DEV)].contiguous().view(-1)
    s2_obs = obs[perm[-n:].to(DEV)].contiguous().view(-1)
    a = torch.randint(0, 5, (n,), generator=g, dtype=torch.int32).to(DEV)
    r = (torch.randn(n, generator=g) * 300).to(DEV)
    d = (torch.rand(n, generator=g) < 0.2).to(torch.uint8).to(DEV)
    return s_obs, s2_obs, a, r, d


def _window_of(stats):
    f = stats.fields()
    out = []
    for g in range(stats.nets):
        w = {k: f[k][g] for k in lu.I64 + lu.SUMS + lu.EXT}
        w["act_hist"], w["td_hist"] = np.array(f["act_hist"][g]), np.array(f["td_hist"][g])
        out.append(w)
    return out


def _check_stats(stats, want, what):
    for g, (got, w) in enumerate(zip(_window_of(stats), want)):
        for k in lu.I64:
            assert int(got[k]) == int(w[k]), (what, g, k, got[k], w[k])
        for k in ("act_hist", "td_hist"):
            assert np.array_equal(got[k], w[k]), (what, g, k)
        for k in lu.SUMS + lu.EXT:
            assert _same_f64(got[k], w[k]), (what, g, k, got[k], float(w[k]))


def _restate_learner(lr, nets, max_norm):
    """The window one learn step must leave, from the learner's own buffers and batch."""
    Q, Qt, a, r, done, sel, grow, B = lr.stat_batch
    A = 5
    h = dict(Q=Q.cpu().numpy().reshape(nets * B, A), Qt=Qt.cpu().numpy().reshape(nets * B, A), a=a.cpu().numpy(),
             r=r.cpu().numpy(), done=done.cpu().numpy(), sel=None if sel is None else sel.cpu().numpy(),
             grow=None if grow is None else grow.cpu().numpy())
    loss, norm = lr.loss.cpu().numpy(), lr.norm.cpu().numpy()
    want, douts = [], []
    for g in range(nets):
        s = slice(g * B, (g + 1) * B)
        w = lu.empty_window()
        douts.append(lu.fold(w, h["Q"][s], h["Qt"][s], h["a"][s], h["r"][s], h["done"][s], F32(lr.gamma),
                             sel=None if h["sel"] is None else h["sel"][s],
                             gamma_row=None if h["grow"] is None else h["grow"][s], loss=loss[g], norm=norm[g],
                             max_norm=max_norm))
        assert _same_f64(w["s_loss"], np.float64(loss[g])) and _same_f64(w["s_norm"], np.float64(norm[g]))
        want.append(w)
    return want, np.concatenate(douts)


@pytest.mark.parametrize("B,fused", [(64, True), (256, True), (64, False)])
def test_fused_learner_statistics_match_and_change_nothing(small_env, B, fused):
    from evacx.lstats import LearnStats
    from evacx.qnet import Learner
    lay, env = small_env
    runs = []
    for with_stats in (True, False):
        stats = LearnStats(1, DEV) if with_stats else None
        lr = Learner(kind="mlp", precision="f32", seed=21, lr=1e-3, stats=stats)
        assert lr.fused_opt
        lr.fused_opt = fused
        g = torch.Generator().manual_seed(4)
        s_obs, s2_obs, a, r, d = _batch(env, lay, B, g)
        lr.learn_obs(lay.c, s_obs, a, r, d, s2_obs, B)
        _sync()
        runs.append(lr)
    on, off = runs
    assert off.stats is None and off.stat_batch is None
    for x, y in ((on.online.flat, off.online.flat), (on.m, off.m), (on.v, off.v), (on.loss, off.loss),
                 (on.norm, off.norm), (on.grads.flat, off.grads.flat)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    want, _ = _restate_learner(on, 1, 1.0)
    assert want[0]["rows"] == B and want[0]["rows_bad"] == 0 and want[0]["steps"] == 1
    _check_stats(on.stats, want, f"fused={fused} B={B}")
    assert _same_f64(on.stats.s_loss.cpu().numpy(), on.loss.double().cpu().numpy())
    assert _same_f64(on.stats.s_norm.cpu().numpy(), on.norm.double().cpu().numpy())
    s = on.stats.summary()
    assert s["steps"] == 1 and s["rows"] == B and s["loss_mean"] == float(on.loss.item())
    assert s["clipped_frac"] == float(on.norm.item() > 1.0) and abs(sum(s["action_frac"]) - 1.0) < 1e-12
    assert on.stats.summary()["steps"] == 0 and on.stats.summary()["q_mean"] is None  # cleared


def test_options_reach_the_statistics_and_d_is_the_chains_td_error(small_env):
    """double_q + Huber + a gamma_row: the target uses last_sel and the row discounts, and |d_out| is
    the td_abs the learn chain itself wrote, bit for bit (one expression in both kernels)."""
    from evacx.lstats import LearnStats
    from evacx.qnet import Learner
    lay, env = small_env
    B = 256
    for fused in (True, False):
        stats = LearnStats(1, DEV)
        lr = Learner(kind="mlp", precision="f32", seed=22, lr=1e-3, double_q=True, loss="huber", huber_delta=10,
                     stats=stats)
        lr.fused_opt = fused
        g = torch.Generator().manual_seed(6)
        s_obs, s2_obs, a, r, d = _batch(env, lay, B, g)
        grow = (0.99 ** torch.randint(1, 6, (B,), generator=g).float()).to(DEV)
        td = torch.zeros(B, dtype=torch.float32, device=DEV)
        lr.learn_obs(lay.c, s_obs, a, r, d, s2_obs, B, td_abs=td, gamma_row=grow)
        _sync()
        Q, Qt, a_, r_, d_, sel, grow_, B_ = lr.stat_batch
        assert sel is lr.last_sel and sel is not None and grow_ is grow
        want, ref_d = _restate_learner(lr, 1, 1.0)
        _check_stats(stats, want, f"options fused={fused}")
        # without the options the restated target differs: they did reach the statistics
        plain = lu.empty_window()
        lu.fold(plain, Q.cpu().numpy(), Qt.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), F32(0.99))
        assert not _same_f64(plain["s_y"], want[0]["s_y"])
        probe = LearnStats(1, DEV)
        dout = torch.zeros(B, dtype=torch.float32, device=DEV)
        probe.update(Q, Qt, a_, r_, d_, lr.gamma, B, sel=sel, gamma_row=grow_, d_out=dout)
        _sync()
        assert torch.equal(dout.abs().view(torch.int32), td.view(torch.int32))
        assert np.array_equal(dout.cpu().numpy().view(np.uint32), ref_d.view(np.uint32))


def test_dense_learner_statistics_match_and_change_nothing():
    _need_gpu()
    from evacx.lstats import LearnStats
    from evacx.qnet import Learner
    B = 32
    g = torch.Generator().manual_seed(12)
    x = (torch.rand(B, 11, 11, 6, generator=g) < 0.3).float().to(DEV)
    x2 = (torch.rand(B, 11, 11, 6, generator=g) < 0.3).float().to(DEV)
    a = torch.randint(0, 5, (B,), generator=g, dtype=torch.int32).to(DEV)
    r = (torch.randn(B, generator=g) * 300).to(DEV)
    d = (torch.rand(B, generator=g) < 0.2).to(torch.uint8).to(DEV)
    m1, m2 = ((torch.rand(B, 512, generator=g) >= 0.2).to(torch.uint8).to(DEV) for _ in range(2))
    runs = []
    for with_stats in (True, False):
        lr = Learner(kind="mlp", precision="exact", seed=5, lr=1e-3, stats=LearnStats(1, DEV) if with_stats else None)
        assert lr.fast is None
        lr.learn(x, a, r, d, x2, m1, m2)
        _sync()
        runs.append(lr)
    on, off = runs
    for p, q in ((on.online.flat, off.online.flat), (on.m, off.m), (on.v, off.v), (on.loss, off.loss)):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    want, _ = _restate_learner(on, 1, 1.0)
    assert want[0]["rows"] == B
    _check_stats(on.stats, want, "dense")


def test_grouped_learner_statistics_match_and_change_nothing(small_env):
    from evacx.lstats import LearnStats
    from evacx.qgroup import GroupedLearner
    lay, env = small_env
    G, B = 3, 64
    runs = []
    for with_stats in (True, False):
        gl = GroupedLearner(G, DEV, lr=1e-3, seed=31, stats=LearnStats(G, DEV) if with_stats else None)
        g = torch.Generator().manual_seed(8)
        s_obs, s2_obs, a, r, d = _batch(env, lay, G * B, g)
        gl.learn_obs(lay.c, s_obs, a, r, d, s2_obs, B)
        _sync()
        runs.append(gl)
    on, off = runs
    for p, q in ((on.flat, off.flat), (on.m, off.m), (on.v, off.v), (on.loss, off.loss), (on.norm, off.norm)):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    want, _ = _restate_learner(on, G, 1.0)
    assert [w["rows"] for w in want] == [B] * G
    _check_stats(on.stats, want, "grouped")
    s = on.stats.summary()
    assert s["steps"] == 1 and s["rows"] == G * B and len(s["per_net"]) == G and s["per_net"][1]["rows"] == B
    assert s["per_net"][2]["loss_mean"] == float(on.loss[2].item())


# ------------------------------------------------------------------ 3. evx_vprobe_*
def _probe_arrays(vp):
    return {k: getattr(vp, k).cpu().numpy() for k in lu.VP_FIELDS}


def _check_probe(vp, st, what):
    got = _probe_arrays(vp)
    for k in lu.VP_FIELDS:
        same = _same_f64(got[k], st[k]) if got[k].dtype == np.float64 else np.array_equal(got[k], st[k])
        assert same, (what, k, got[k][:8], st[k][:8])


def _check_rows(host_rows, want, what):
    i, f = host_rows.numpy(), host_rows.numpy().view(np.float64)
    for k, w in enumerate(want):
        assert tuple(int(v) for v in i[k][:3]) == w[:3], (what, k, i[k][:3], w[:3])
        assert _same_f64(f[k][3:], np.array(w[3:])), (what, k, f[k][3:], w[3:])


@pytest.mark.parametrize("R", [1, 2, 16])
@pytest.mark.parametrize("E", [1, 7, 1025])
def test_vprobe_matches_the_float64_loop(E, R):
    _need_gpu()
    from evacx.lstats import ValueProbe
    A, gamma, steps = 5, 0.99, 40
    rng = np.random.RandomState(100 * E + R)
    li = (np.arange(E) % 2).astype(np.int32)
    vp = ValueProbe(E, R, DEV, gamma, layout_idx=_dev(li), n_layouts=2)
    halves = ValueProbe(E, R, DEV, gamma)  # the same steps through two views
    lo_n = E // 2
    parts = [halves.view(0, lo_n), halves.view(lo_n, E - lo_n)] if lo_n else [halves]
    st = lu.probe_state(E)
    _check_probe(vp, st, "init")
    for t in range(steps):
        Q = (rng.randn(E * R, A) * 1e4).astype(F32)
        Q[rng.rand(E * R) < 0.01, :] = np.inf  # a non-finite Q0 now and then
        act = rng.randint(-1, A + 1, size=E * R).astype(np.int32)
        rew = rng.randn(E) * 300
        done = (rng.rand(E) < 0.1).astype(np.uint8)
        dQ, dact, drew, ddone = _dev(Q), _dev(act), _dev(rew), _dev(done)
        vp.update(dQ, dact, drew, ddone)
        bounds = [(0, lo_n), (lo_n, E - lo_n)] if lo_n else [(0, E)]
        for part, (lo, n) in zip(parts, bounds):
            part.update(dQ[lo * R:(lo + n) * R].contiguous(), dact[lo * R:(lo + n) * R].contiguous(),
                        drew[lo:lo + n].contiguous(), ddone[lo:lo + n].contiguous())
        lu.probe_step_vec(st, Q, act, rew, done, gamma, R)
        _check_probe(vp, st, f"step {t}")
    _check_probe(halves, st, "two half views")
    if E > 1:
        assert st["w_n"].sum() > 0 and st["open"].sum() > 0
    if E == 1025:
        assert st["w_bad"].sum() > 0  # a non-finite Q0 landed in w_bad (and, by the loop, nowhere else)
    want = lu.probe_rows(st, li, 2)
    _check_rows(vp.reduce(clear=False), want, "reduce")
    s = vp.summary(clear=True)  # clear keeps the probes in progress
    assert (s["probes"], s["bad"], s["open"]) == want[2][:3] and len(s["per_layout"]) == 2
    if s["probes"]:
        assert s["bias"] == want[2][5] / s["probes"]
    for k in ("w_n", "w_bad"):
        st[k][:] = 0
    for k in ("w_q", "w_g", "w_e", "w_e2", "w_q2", "w_g2", "w_qg"):
        st[k][:] = 0.0
    st["w_emin"][:], st["w_emax"][:] = np.inf, -np.inf
    _check_probe(vp, st, "after clear")
    assert vp.summary(clear=False)["open"] == int(st["open"].sum())
    # discard closes the masked probes without folding them
    mask = rng.rand(E) < 0.5
    mask[0] = True
    vp.discard(_dev(mask))
    st["open"][mask] = 0
    _check_probe(vp, st, "after discard")
    s = vp.summary(clear=False)
    assert s["probes"] == 0 and s["bad"] == 0 and s["open"] == int(st["open"].sum())
    vp.discard()
    assert vp.summary()["open"] == 0


# ------------------------------------------------------------------ 4. the trainer
@pytest.fixture(scope="module")
def trainer_layout():
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    return DeviceLayout(build_tables(synthetic(64, 64, 4)), 300)


def _make(lay, E=64, **kw):
    from evacx.trainer import VecTrainer
    args = dict(batch=256, replay_capacity=4096, target_every=5, lr=1e-3)
    args.update(kw)
    return VecTrainer(lay, E, **args)


def _finish(tr):
    tr.sync()
    _sync()
    tr.env.check_err()


def _nets(tr):
    """(online, target, m, v) flat tensors of either learner kind."""
    if tr.learner is not None:
        return tr.learner.online.flat, tr.learner.target.flat, tr.learner.m, tr.learner.v
    return tr.glearner.flat, tr.glearner.tflat, tr.glearner.m, tr.glearner.v


SCHEDULES = {"strict": dict(), "prioritized": dict(replay="prioritized"), "lagged": dict(lagged_learn=True),
             "per_robot": dict(nets="per_robot")}


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_trainer_diagnostics_only_read(trainer_layout, name):
    lay, kw, steps, R = trainer_layout, SCHEDULES[name], 30, 4
    on = _make(lay, learn_stats=True, value_probe=True, **kw)
    off = _make(lay, **kw)
    assert off.learn_stats is None and off.probe is None and off.act_q is None
    assert all(g.probe is None and g.q is None for g in off.groups)
    st = lu.probe_state(64)
    for t in range(steps):
        on.step()
        off.step()
        on.sync()
        _sync()
        # the host loop over this step's Q, actions, reward and done reproduces the device's probe state
        lu.probe_step_vec(st, on.act_q.cpu().numpy().reshape(-1, 5), on.actions.cpu().numpy(),
                          on.env.reward.cpu().numpy(), on.env.done.cpu().numpy(), on.probe.gamma, R)
        if t == 0:
            assert on.probe.open.cpu().numpy().all()  # every env has an open probe after the first step
        _check_probe(on.probe, st, f"{name} step {t}")
    _finish(on)
    _finish(off)
    for x, y in zip(_nets(on), _nets(off)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert on.learn_steps == off.learn_steps and on.learn_steps >= 20
    assert torch.equal(on.last_loss.view(torch.int32), off.last_loss.view(torch.int32))
    assert torch.equal(on.actions, off.actions) and torch.equal(on.env.obs, off.env.obs)
    for k in ("r", "a", "done"):
        x, y = getattr(on.replay, k), getattr(off.replay, k)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), k
    s = on.learn_summary(clear=False)
    assert s["steps"] == on.learn_steps
    assert s["rows"] == s["steps"] * 256 and s["rows_bad"] == 0 and s["steps_bad"] == 0
    assert s["td_p50"] <= s["td_p90"] <= s["td_p99"] and s["td_abs_mean"] <= s["td_abs_max"]
    assert s["q_min"] <= s["q_mean"] <= s["qmax_mean"] <= s["q_max"]
    if name == "per_robot":
        assert len(s["per_net"]) == R and all(p["rows"] == s["steps"] * 64 for p in s["per_net"])
    v = on.value_summary(clear=False)
    assert v["open"] == int(st["open"].sum()) and v["probes"] == int(st["w_n"].sum())
    with pytest.raises(RuntimeError):
        off.learn_summary()
    with pytest.raises(RuntimeError):
        off.value_summary()


def test_trainer_probe_counts_the_episodes_and_qmix_runs():
    """A 24 x 20 layout of 60 people ends its episodes in about 60 steps: over 150 steps every folded or
    bad probe is one episode EpisodeStats counted. nets="qmix" takes the probe (not the statistics)."""
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    lay = DeviceLayout(build_tables(synthetic(24, 20, 4)), 60)
    tr = _make(lay, value_probe=True, episode_stats=True, act_table=False)
    for _ in range(150):
        tr.step()
    _finish(tr)
    e, v = tr.episode_summary(clear=False), tr.value_summary(clear=False)
    assert e["episodes"] > 0 and v["probes"] + v["bad"] == e["episodes"], (e["episodes"], v["probes"], v["bad"])
    assert v["bad"] == 0 and v["open"] == 64 - int(tr.env.done.sum())
    assert v["rmse"] >= abs(v["bias"]) * (1 - 1e-12) and v["err_min"] <= v["bias"] <= v["err_max"]
    mask = torch.zeros(64, dtype=torch.bool, device=DEV)
    mask[::2] = True
    tr.step(extra_reset=mask)  # a forced reset closes the masked probes without a pair
    _finish(tr)
    after = tr.value_summary(clear=False)
    closed = int((mask & ~tr.env.done.bool()).sum())
    assert closed > 0 and after["open"] == 64 - closed - int(tr.env.done.sum())
    assert after["probes"] + after["bad"] == tr.episode_summary(clear=False)["episodes"]
    qm = _make(lay, nets="qmix", value_probe=True, act_table=False)
    for _ in range(12):
        qm.step()
    _finish(qm)
    assert qm.learn_stats is None and qm.value_summary()["open"] == 64 and torch.isfinite(qm.act_q).all()


# ------------------------------------------------------------------ 5. the runner
def test_train_vec_learn_stats_writes_its_log_and_leaves_the_training_log_alone(tmp_path, capsys):
    _need_gpu()
    from Louvre_Evacuation.runners import train_vec
    cfg = tmp_path / "small.yaml"
    cfg.write_text("env:\n  width: 36\n  height: 30\n  fire_zones: [[18, 14]]\n  exit_location: [36, 15]\n"
                   "  num_people: 40\nagent:\n  gamma: 0.99\n  epsilon: 1.0\n  epsilon_min: 0.02\n"
                   "  epsilon_decay: 0.9995\n  learning_rate: 0.0001\n  batch_size: 32\n  target_update_freq: 20\n"
                   "  memory_size: 4096\nsave_path: \"unused\"\n")
    logs = {}
    for flag in (True, False):
        out = tmp_path / ("on" if flag else "off")
        argv = ["--config", str(cfg), "--envs", "64", "--steps", "60", "--log-every", "20", "--out", str(out)]
        train_vec.train_vec(train_vec.parse_args(argv + (["--learn-stats"] if flag else [])))
        logs[flag] = (out / "training_log.csv").read_bytes()
        assert (out / "learn_log.csv").exists() == flag
    assert logs[True] == logs[False] and logs[True].count(b"\n") == 4
    rows = list(csv.reader(open(tmp_path / "on" / "learn_log.csv")))
    assert rows[0] == train_vec.LEARN_COLUMNS and [r[0] for r in rows[1:]] == ["20", "40", "60"]
    assert all(len(r) == len(train_vec.LEARN_COLUMNS) for r in rows)
    assert sum(int(r[1]) for r in rows[-1:]) > 0 and float(rows[-1][2]) == float(rows[-1][2])  # q_mean is a number
    assert rows[-1][15] == "0" and rows[-1][16] == "0"
    assert capsys.readouterr().out.count("learn: q=") == 3
