"""Terminal health on the device (csrc/health.hip, evacx.health), evaluate(metrics=True), the
per-robot greedy policies and the evaluate_vec runner.

The reference everywhere is numpy on the host -- np.mean / min over the not-dead persons'
healths in person order, sequential f64 folds per env, the reduce's order restated -- never
HealthStats itself. Every f64 is compared bit for bit (NaN against NaN where nobody is alive)."""
import csv

import numpy as np
import pytest
import torch

import health_util as hu
from span_reduce_util import span_min, span_sum

pytestmark = pytest.mark.gpu

DEAD = 1 << 25    # pk: the person is dead
SAFE = 1 << 24    # pk: the person is evacuated


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same(got, want):
    """f64 arrays equal bit for bit, NaN matching NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(hu.bits(got[~nan]), hu.bits(want[~nan]))


def _metrics(pk_row, health_row):
    """get_performance_metrics' three numbers of one env (envs/evacuation_env.py:290-309)."""
    alive = [float(h) for h, p in zip(health_row, pk_row) if not p & DEAD]
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            avg = float(np.mean(alive))
    return avg, float(min(alive, default=100)), len(alive)


def _kill(rng, P, n_alive):
    """A dead mask that leaves n_alive persons, at random places."""
    dead = np.ones(P, bool)
    dead[rng.choice(P, n_alive, replace=False)] = False
    return dead


def _case(P):
    """pk [16, P] (positions in the low bits), health [16, P], done [16] for one P."""
    E = 16
    rng = np.random.default_rng(500 + P)
    pk = (rng.integers(1, 60, (E, P)) | (rng.integers(1, 60, (E, P)) << 12)).astype(np.int64)
    health = rng.random((E, P)) * 100
    dead = np.zeros((E, P), bool)
    dead[1] = True                                  # all dead: nan, 100.0, 0
    dead[2, :-1] = True                             # only the last person alive
    dead[3, ::2] = True                             # alternating
    dead[4] = rng.random(P) < 1 / 3                 # a random third dead
    pk[5] |= np.where(rng.random(P) < 0.5, SAFE, 0)  # evacuated persons count ...
    dead[5] = rng.random(P) < 0.25                  # ... also next to dead ones
    dead[6] = rng.random(P) < 0.5                   # done == 0: must stay untouched
    dead[8, 1::2] = True                            # alternating, the other half
    for e in range(9, E):
        dead[e] = rng.random(P) < rng.random()
    if P == 1000:
        for e, n in zip((9, 10, 11, 12), (127, 128, 129, 257)):
            dead[e] = _kill(rng, P, n)
    if P == 9102:  # the CPU test's inputs: the two sizes past one chunk of numpy's reduction
        health[0] = hu.healths(9102)
        dead[9] = _kill(rng, P, 8193)
        health[9, ~dead[9]] = hu.healths(8193)
    pk = (pk | np.where(dead, DEAD, 0)).astype(np.uint32).view(np.int32)
    done = np.ones(E, np.uint8)
    done[6] = 0
    return pk, health, done


@pytest.mark.parametrize("P", [7, 150, 300, 1000, 9102])
def test_kernel_equals_numpy_bit_for_bit(P):
    _need_gpu()
    from evacx.health import HealthStats
    pk, health, done = _case(P)
    E = len(done)
    st = HealthStats(E, "cuda", P, record=1)
    st.last_avg.fill_(-7.0)  # a sentinel the done == 0 env must keep
    st.update((torch.from_numpy(pk).cuda().view(-1), torch.from_numpy(health).cuda().view(-1)),
              torch.from_numpy(done).cuda())
    torch.cuda.synchronize()
    want = [_metrics(pk[e].view(np.uint32), health[e]) for e in range(E)]
    avg, mn, alive = (st.last_avg.cpu().numpy(), st.last_min.cpu().numpy(), st.last_alive.cpu().numpy())
    for e in range(E):
        print(f"P={P} env {e}: alive {alive[e]} avg {avg[e]!r} (numpy {want[e][0]!r}) min {mn[e]!r}")
    on = done.astype(bool)
    assert _same(avg[on], [w[0] for w, d in zip(want, on) if d])
    assert _same(mn[on], [w[1] for w, d in zip(want, on) if d])
    assert np.array_equal(alive[on], [w[2] for w, d in zip(want, on) if d])
    assert np.isnan(avg[1]) and mn[1] == 100.0 and alive[1] == 0
    assert alive[2] == 1 and avg[2] == health[2, -1] == mn[2]
    assert alive[0] == P
    # the table's slot 0 and the lifetime count follow; the done == 0 env is untouched
    assert _same(st.tab_avg.cpu().numpy()[on, 0], avg[on]) and _same(st.tab_min.cpu().numpy()[on, 0], mn[on])
    assert np.array_equal(st.tab_alive.cpu().numpy()[on, 0], alive[on])
    assert st.n_total.cpu().tolist() == [int(d) for d in done]
    assert avg[6] == -7.0 and mn[6] == 0.0 and alive[6] == 0 and st.w_n[6].item() == 0
    assert st.tab_avg[6, 0].item() == 0.0 and st.w_lo[6].item() == float("inf")
    if P == 9102:  # the order is numpy's chunked one, not plain pairwise over the whole list
        from oracle import oracle as orc
        assert alive[9] == 8193
        for e, n in ((0, 9102), (9, 8193)):
            assert hu.bits(avg[e]) == hu.bits(np.mean(hu.healths(n)))
            assert hu.bits(avg[e]) != hu.bits(orc.pairwise_sum(hu.healths(n)) / n)


def test_window_cap_table_and_lifetime_match_a_numpy_fold():
    _need_gpu()
    from evacx.health import HealthStats
    E, P, steps, cap, K = 16, 150, 24, 2, 3
    rng = np.random.default_rng(77)
    st = HealthStats(E, "cuda", P, cap=cap, record=K)
    f = dict(n_total=np.zeros(E, np.int64), w_n=np.zeros(E, np.int64), w_has=np.zeros(E, np.int64),
             w_alive=np.zeros(E, np.int64), w_avg=np.zeros(E), w_min=np.zeros(E), w_lo=np.full(E, np.inf),
             last_avg=np.zeros(E), last_min=np.zeros(E), last_alive=np.zeros(E, np.int64))
    tab = dict(tab_avg=np.zeros((E, K)), tab_min=np.zeros((E, K)), tab_alive=np.zeros((E, K), np.int64))
    for t in range(steps):
        health = rng.random((E, P)) * 100
        dead = rng.random((E, P)) < rng.random((E, 1))
        dead[t % E] = True  # an episode that nobody survives: no avg_health, min_health 100
        pk = np.where(dead, DEAD, 0).astype(np.uint32).view(np.int32)
        done = (rng.random(E) < 0.5).astype(np.uint8)
        done[t % E] = 1
        st.update((torch.from_numpy(pk).cuda().view(-1), torch.from_numpy(health).cuda().view(-1)),
                  torch.from_numpy(done).cuda())
        for e in np.nonzero(done)[0]:
            avg, mn, n = _metrics(pk[e].view(np.uint32), health[e])
            k = f["n_total"][e]
            if k < cap:
                f["w_n"][e] += 1
                f["w_alive"][e] += n
                if n > 0:
                    f["w_has"][e] += 1
                    f["w_avg"][e] = f["w_avg"][e] + avg
                f["w_min"][e] = f["w_min"][e] + mn
                f["w_lo"][e] = min(f["w_lo"][e], mn)
            f["last_avg"][e], f["last_min"][e], f["last_alive"][e] = avg, mn, n
            if k < K:
                tab["tab_avg"][e, k], tab["tab_min"][e, k], tab["tab_alive"][e, k] = avg, mn, n
            f["n_total"][e] = k + 1
    torch.cuda.synchronize()
    assert (f["n_total"] > K).any() and (f["n_total"] >= cap).all() and (f["w_has"] < f["w_n"]).any()
    for k, want in {**f, **tab}.items():
        got = getattr(st, k).cpu().numpy()
        assert _same(got, want) if want.dtype == np.float64 else np.array_equal(got, want), k
    assert (st.w_n.cpu().numpy() == cap).all()
    s = st.summary(clear=True)
    assert s["episodes"] == cap * E and s["health_episodes"] == int(f["w_has"].sum())
    assert s["min_health"] == f["w_lo"].min() and s["alive_mean"] == int(f["w_alive"].sum()) / (cap * E)
    # cleared: the window is empty, the last-episode slots, the table and the lifetime count stay
    s2 = st.summary(clear=False)
    assert s2["episodes"] == 0 and s2["avg_health"] is None and s2["min_health"] is None
    assert np.array_equal(st.n_total.cpu().numpy(), f["n_total"]) and _same(st.last_avg.cpu().numpy(), f["last_avg"])
    assert _same(st.tab_avg.cpu().numpy(), tab["tab_avg"]) and (st.w_lo.cpu().numpy() == np.inf).all()


def test_reduce_adds_in_the_stated_order():
    _need_gpu()
    from evacx.health import ROW_WORDS, HealthStats
    E, nl = 2500, 3  # 2500 > 2 * SPAN: a reduce thread adds up to three envs
    rng = np.random.default_rng(31)
    lidx = rng.integers(0, nl, E).astype(np.int32)
    st = HealthStats(E, "cuda", 150, layout_idx=torch.from_numpy(lidx).cuda(), n_layouts=nl)
    w = dict(w_n=rng.integers(0, 5, E), w_has=rng.integers(0, 4, E), w_alive=rng.integers(0, 600, E),
             w_avg=rng.random(E) * 400 * np.exp(rng.uniform(-3, 3, E)), w_min=rng.random(E) * 400,
             w_lo=rng.random(E) * 100)
    for k, v in w.items():
        getattr(st, k).copy_(torch.from_numpy(v))
    s = st.summary(clear=False)
    rows = st.rows.cpu().clone()
    irow = rows.view(nl + 1, ROW_WORDS).numpy()
    frow = rows.view(torch.float64).view(nl + 1, ROW_WORDS).numpy()
    for r in range(nl + 1):
        member = np.ones(E, bool) if r == nl else lidx == r
        assert irow[r, 0] == w["w_n"][member].sum() and irow[r, 1] == w["w_has"][member].sum()
        assert irow[r, 2] == w["w_alive"][member].sum()
        assert hu.bits(frow[r, 3]) == hu.bits(span_sum(w["w_avg"], member)), r
        assert hu.bits(frow[r, 4]) == hu.bits(span_sum(w["w_min"], member)), r
        assert frow[r, 5] == w["w_lo"][member].min() == span_min(w["w_lo"], member), r
    assert s["episodes"] == int(w["w_n"].sum()) and len(s["per_layout"]) == nl
    assert sum(p["episodes"] for p in s["per_layout"]) == s["episodes"]
    assert s["avg_health"] == frow[nl, 3] / irow[nl, 1] and s["min_health_mean"] == frow[nl, 4] / irow[nl, 0]
    st.summary(clear=False)
    assert torch.equal(rows, st.rows.cpu())  # a second run: the same bits


# ------------------------------------------------------------------ evaluate(metrics=True)
def _layout(R=1, P=150):
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, reference_multi, synthetic
    return DeviceLayout(build_tables(synthetic(36, 30, 1) if R == 1 else reference_multi()), P)


def _tables_equal(a, b, keys=None):
    for k in (keys or a["per_env"]):
        x, y = a["per_env"][k], b["per_env"][k]
        same = torch.equal(x.view(torch.int64), y.view(torch.int64)) if x.dtype == torch.float64 else torch.equal(x, y)
        assert same, k


def test_evaluate_metrics_match_a_host_loop_and_leave_the_trajectory_alone():
    _need_gpu()
    from evacx.env import VecEnv
    from evacx.evaluate import evaluate
    P, E, action = 150, 8, 4
    lay = _layout()
    off = evaluate(lay, E, 1, action)
    on = evaluate(lay, E, 1, action, metrics=True)
    # everything metrics=False returns is unchanged
    for k in off:
        if k == "per_env":
            _tables_equal(off, on, keys=off["per_env"])
        elif k == "per_layout":
            for a, b in zip(off[k], on[k]):
                assert a == {kk: b[kk] for kk in a}
        else:
            assert off[k] == on[k], k
    assert set(on) - set(off) == {"avg_health", "min_health", "min_health_mean", "alive_mean", "health_episodes",
                                  "total_time_mean"}
    assert on["total_time_mean"] == on["length_mean"] * 0.5
    # the host loop: separate resets, np.mean / min from the downloaded state at every done
    env = VecEnv(lay, E)
    env.seed([1234 + i for i in range(E)])
    env.reset()
    a = torch.full((E * lay.R,), action, dtype=torch.int32, device="cuda")
    first = {}
    for t in range(on["steps"]):
        env.step(a, auto_reset=False)
        done = env.done.cpu().numpy().astype(bool)
        if done.any():
            ids = np.nonzero(done)[0].tolist()
            for e, hs in zip(ids, env.host_states(ids)):
                alive = [float(h) for h, fl in zip(hs["health"], hs["flags"]) if not fl & 2]
                first.setdefault(e, (float(np.mean(alive)) if alive else float("nan"), min(alive, default=100),
                                     len(alive)))
            env.reset(mask=env.done)
    env.check_err()
    assert sorted(first) == list(range(E))
    tab = {k: on["per_env"][k].cpu().numpy()[:, 0] for k in ("tab_avg_health", "tab_min_health", "tab_alive")}
    for e in range(E):
        print(f"env {e}: device {tab['tab_avg_health'][e]!r} {tab['tab_min_health'][e]!r} {tab['tab_alive'][e]} "
              f"host {first[e]}")
    assert _same(tab["tab_avg_health"], [first[e][0] for e in range(E)])
    assert _same(tab["tab_min_health"], [first[e][1] for e in range(E)])
    assert np.array_equal(tab["tab_alive"], [first[e][2] for e in range(E)])
    has = [first[e][0] for e in range(E) if first[e][2] > 0]
    assert on["health_episodes"] == len(has)
    assert on["min_health"] == min(first[e][1] for e in range(E))
    assert on["alive_mean"] == sum(first[e][2] for e in range(E)) / E
    if has:
        # E = 8 <= SPAN: 0.0 + v per thread (exact), then a pairwise tree of depth 3 over n values <= 100:
        # |sum - fsum| <= 3 * 2^-53 * 100 n, so the means differ by at most 150 * 2^-52, plus one rounding
        # of each division (2^-53 * 100 each): 250 * 2^-52, rounded up to 256
        import math
        assert abs(on["avg_health"] - math.fsum(has) / len(has)) <= 2.0 ** -52 * 256.0


# ------------------------------------------------------------------ per-robot policies
_POL = {}


def _policy_runs():
    """The evaluations the policy tests share (two-robot 36x30, 8 envs, 1 episode each)."""
    if not _POL:
        from evacx.evaluate import evaluate
        from evacx.qgroup import GroupedLearner, GroupedQMix
        from evacx.qnet import Learner
        lay = _layout(R=2)
        assert lay.R == 2
        one = Learner(kind="mlp", precision="f32", seed=5)  # no act table attached
        grp = GroupedLearner(2, init_seeds=[3, 4])
        _POL.update(lay=lay, one=one, grp=grp,
                    single=evaluate(lay, 8, 1, "greedy", learner=one),
                    twice=evaluate(lay, 8, 1, "greedy", learner=[one, one]),
                    grouped=evaluate(lay, 8, 1, "greedy", learner=grp),
                    each=evaluate(lay, 8, 1, "greedy", learner=[Learner(seed=3), Learner(seed=4)]),
                    qmix=evaluate(lay, 8, 1, "greedy", learner=GroupedQMix(grp)))
    return _POL


def _same_eval(a, b):
    _tables_equal(a, b)
    assert {k: v for k, v in a.items() if k not in ("per_env", "per_layout")} == \
        {k: v for k, v in b.items() if k not in ("per_env", "per_layout")}


def test_a_sequence_of_one_learner_twice_equals_the_shared_learner():
    _need_gpu()
    r = _policy_runs()
    assert r["single"]["episodes"] == 8
    _same_eval(r["single"], r["twice"])


def test_a_sequence_without_the_fused_act_equals_the_shared_learner():
    """Learners without a fused act (conv agents; here the MLP on the exact-f32 GEMMs, which add over
    K in one order whatever the row count) go through q_values + evx_act per robot."""
    _need_gpu()
    from evacx.evaluate import evaluate
    from evacx.qnet import Learner
    lay = _policy_runs()["lay"]
    ex = Learner(kind="mlp", precision="exact", seed=6)
    assert ex.fast is None
    _same_eval(evaluate(lay, 8, 1, "greedy", learner=ex), evaluate(lay, 8, 1, "greedy", learner=[ex, ex]))


def test_grouped_learner_equals_one_learner_per_robot_and_qmix_its_agents():
    _need_gpu()
    r = _policy_runs()
    assert r["grouped"]["episodes"] == 8
    _same_eval(r["grouped"], r["each"])
    _same_eval(r["grouped"], r["qmix"])


def test_grouped_load_state_dict_round_trips_and_refuses_a_wrong_shape():
    _need_gpu()
    from evacx.qgroup import GroupedLearner
    grp = _policy_runs()["grp"]
    other = GroupedLearner(2, init_seeds=[9, 10])
    sd = {k: v.cpu() for k, v in grp.state_dict(0).items()}  # as loaded from a checkpoint
    other.load_state_dict(1, sd)
    torch.cuda.synchronize()
    assert torch.equal(other.flat[1].view(torch.int32), grp.flat[0].view(torch.int32))
    assert not torch.equal(other.flat[0], grp.flat[0])
    for k, buf in grp.fast.bufs.items():  # the repacked operands of the act
        assert torch.equal(other.fast.bufs[k][1], buf[0]), k
    back = other.state_dict(1)
    for k in sd:
        assert torch.equal(back[k].cpu().view(torch.int32), sd[k].view(torch.int32)), k
    bad = dict(sd)
    bad["fc1.weight"] = torch.zeros(512, 725)
    with pytest.raises(ValueError, match="fc1.weight"):
        other.load_state_dict(0, bad)
    assert torch.equal(other.flat[1].view(torch.int32), grp.flat[0].view(torch.int32))  # nothing was written


def test_per_robot_policies_refuse_wrong_counts_odd_envs_and_other_devices():
    _need_gpu()
    import types
    from evacx.evaluate import evaluate
    from evacx.qgroup import GroupedLearner
    r = _policy_runs()
    lay, one = r["lay"], r["one"]
    with pytest.raises(ValueError, match="learner"):
        evaluate(lay, 8, 1, "greedy", learner=[one])
    with pytest.raises(ValueError, match="learner"):
        evaluate(lay, 8, 1, "greedy", learner=[one, one, one])
    with pytest.raises(ValueError, match="learner"):
        evaluate(lay, 8, 1, "greedy", learner=GroupedLearner(3))
    with pytest.raises(ValueError, match="E"):
        evaluate(lay, 7, 1, "greedy", learner=[one, one])
    with pytest.raises(ValueError, match="E"):
        evaluate(lay, 7, 1, "greedy", learner=r["grp"])
    elsewhere = types.SimpleNamespace(device=torch.device("cpu"))  # refused before it is used
    with pytest.raises(ValueError, match="learner"):
        evaluate(lay, 8, 1, "greedy", learner=[one, elsewhere])


# ------------------------------------------------------------------ runner
def test_evaluate_vec_writes_the_table_evaluate_gives(tmp_path, capsys):
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.evaluate import evaluate
    from evacx.layout import build_tables
    from Louvre_Evacuation.runners import evaluate_vec
    cfg = tmp_path / "small.yaml"
    cfg.write_text("env:\n  width: 36\n  height: 30\n  fire_zones: [[18, 14]]\n  exit_location: [36, 15]\n"
                   "  num_people: 40\nagent:\n  gamma: 0.99\nsave_path: \"unused\"\n")
    out = tmp_path / "out"
    evaluate_vec.main(["--config", str(cfg), "--robots", "2", "--envs", "8", "--episodes", "1", "--out", str(out)])
    text = capsys.readouterr().out
    assert "avg health" in text and "static" in text and "random" in text
    rows = list(csv.reader(open(out / "strategy_comparison.csv")))
    assert rows[0] == evaluate_vec.CSV_COLUMNS and [r[0] for r in rows[1:]] == ["static", "random"]
    lay = DeviceLayout(build_tables(evaluate_vec.build_spec(dict(width=36, height=30, exit_location=[36, 15]), 2)), 40)
    for row, policy in zip(rows[1:], (4, "random")):
        ev = evaluate(lay, 8, 1, policy, metrics=True)
        want = [ev["avg_health"], ev["death_rate"], ev["evac_rate"], ev["total_time_mean"]]
        assert [None if v == "" else float(v) for v in row[1:5]] == want, row
        assert int(row[5]) == ev["episodes"] == 8
        assert format(ev["death_rate"], "10.2%").strip() in text
