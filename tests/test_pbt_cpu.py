"""The exploit / explore scheduler (evacx.pbt.PBTScheduler) on hand-written windows,
and the refusals of evx_copy_members: host logic throughout, no device (the entry validates before
any launch, as tests/test_qmlp_guard_cpu.py's checks do; an address that is never dereferenced
stands in for a device buffer)."""
import ctypes as C
import math

import pytest

K = 8
SPACE = {"lr": ("perturb", (0.8, 1.25), 1e-6, 1e-2)}


def _summary(returns, episodes=None):
    """An episode_summary()-shaped dict: member k finished episodes[k] episodes of return returns[k]."""
    episodes = [4] * len(returns) if episodes is None else episodes
    return {"per_member": [dict(episodes=n, return_sum=r * n, evacuated=10 * n, dead=2 * n)
                           for r, n in zip(returns, episodes)]}


def _hp(**over):
    hp = dict(lr=[1e-3 * (k + 1) for k in range(K)], gamma=[0.99] * K, n_step=[3] * K, target_every=[10] * K,
              loss=["mse"] * K, epsilon=[0.5] * K)
    hp.update(over)
    return hp


def _sched(space=SPACE, **kw):
    from evacx.pbt import PBTScheduler
    return PBTScheduler(kw.pop("members", K), space, **kw)


def _check_map(s, decisions):
    m = s.src_map(decisions)
    assert all(m[m[k]] == m[k] for k in range(len(m))), m  # the kernel's precondition
    assert {d["dst"] for d in decisions}.isdisjoint({d["src"] for d in decisions})
    return m


# ------------------------------------------------------------------ ranking
def test_two_worst_take_from_two_best():
    s = _sched(frac=0.25)
    s.observe(_summary([5.0, 9.0, 1.0, 7.0, 3.0, 8.0, 0.5, 6.0]))
    d = s.plan(_hp())
    assert sorted(x["dst"] for x in d) == [2, 6] and all(x["src"] in (1, 5) for x in d)
    for x in d:
        assert x["fitness_dst"] == [5.0, 9.0, 1.0, 7.0, 3.0, 8.0, 0.5, 6.0][x["dst"]]
        assert x["fitness_src"] == (9.0 if x["src"] == 1 else 8.0)
        assert x["old"] == {"lr": 1e-3 * (x["dst"] + 1)}
        donor = 1e-3 * (x["src"] + 1)
        assert x["new"]["lr"] in (min(max(donor * 0.8, 1e-6), 1e-2), min(max(donor * 1.25, 1e-6), 1e-2))
    m = _check_map(s, d)
    assert [m[k] for k in (0, 1, 3, 4, 5, 7)] == [0, 1, 3, 4, 5, 7]
    assert s.round == 1 and all(w["episodes"] == 0 for w in s.window)


def test_ties_break_by_index():
    s = _sched(frac=0.25)
    s.observe(_summary([1.0] * K))
    d = s.plan(_hp())
    assert sorted(x["dst"] for x in d) == [6, 7] and all(x["src"] in (0, 1) for x in d)
    _check_map(s, d)


def test_ineligible_member_is_neither_donor_nor_receiver():
    """Member 1 (the best return) and member 6 (the worst) have too few episodes; member 4's fitness
    is not finite."""
    s = _sched(frac=0.25, min_episodes=3)
    s.observe(_summary([5.0, 99.0, 1.0, 7.0, math.inf, 8.0, -99.0, 6.0], episodes=[4, 2, 4, 4, 4, 4, 1, 4]))
    assert s.member_fitness(1) is None and s.member_fitness(6) is None and s.member_fitness(4) is None
    d = s.plan(_hp())
    assert sorted(x["dst"] for x in d) == [0, 2] and all(x["src"] in (3, 5) for x in d)
    _check_map(s, d)


def test_q_shrinks_to_half_the_eligible():
    s = _sched(frac=0.5)  # floor(0.5 * 8) = 4, but three eligible members: q = 1
    s.observe(_summary([5.0, 9.0, 1.0, 0, 0, 0, 0, 0], episodes=[4, 4, 4, 0, 0, 0, 0, 0]))
    d = s.plan(_hp())
    assert [(x["dst"], x["src"]) for x in d] == [(2, 1)]
    s.observe(_summary([5.0] + [0] * 7, episodes=[4] + [0] * 7))  # one eligible: nobody moves
    assert s.plan(_hp()) == [] and s.round == 2


def test_empty_plans_still_advance_the_round():
    s = _sched(frac=0.0)
    s.observe(_summary([float(k) for k in range(K)]))
    assert s.plan(_hp()) == [] and s.round == 1 and all(w["episodes"] == 0 for w in s.window)
    s = _sched(frac=0.25)
    s.observe(_summary([1.0] * K, episodes=[0] * K))
    assert s.plan(_hp()) == [] and s.round == 1
    assert s.plan(_hp()) == [] and s.round == 2  # nothing observed at all


def test_observe_adds_windows_and_leaves_the_summary_alone():
    s = _sched()
    summ = _summary([2.0] * K, episodes=[1, 2, 3, 4, 5, 6, 7, 8])
    keep = [dict(r) for r in summ["per_member"]]
    s.observe(summ)
    s.observe(summ)
    assert summ["per_member"] == keep
    assert [w["episodes"] for w in s.window] == [2, 4, 6, 8, 10, 12, 14, 16]
    assert s.window[3] == dict(episodes=8, return_sum=16.0, evacuated=80, dead=16)
    with pytest.raises(ValueError, match="per_member"):
        s.observe({"per_member": keep[:3]})


def test_named_fitnesses_and_a_callable():
    w = {"per_member": [dict(episodes=2, return_sum=3.0, evacuated=30, dead=10)] * 2}
    for fitness, people, want in (("return_mean", None, 1.5), ("evac_rate", 20, 0.75), ("neg_death_rate", 20, -0.25),
                                  ("evac_rate", None, 15.0), (lambda m: m["evacuated"] - m["dead"], None, 20.0)):
        s = _sched(members=2, fitness=fitness, people=people)
        s.observe(w)
        assert s.member_fitness(0) == want
    s = _sched(members=2, fitness=lambda m: float("nan"))
    s.observe(w)
    assert s.member_fitness(0) is None


# ------------------------------------------------------------------ draws
FULL = {"lr": ("perturb", (0.5, 0.8, 1.25, 2.0), 1e-6, 1e-2), "gamma": ("perturb", (0.9, 1.1), 0.5, 0.999),
        "n_step": ("perturb", (0.3, 1.7), 1, 64), "target_every": ("perturb", (0.01, 0.5, 2.0), 0, 1000),
        "loss": ("resample", ("mse", "huber")), "epsilon": ("resample", (0.1, 0.3, 0.9))}
RETURNS = [5.0, 9.0, 1.0, 7.0, 3.0, 8.0, 0.5, 6.0]


def _plans(seed, rounds, space=FULL, frac=0.5):
    s = _sched(space, frac=frac, seed=seed)
    out = []
    for _ in range(rounds):
        s.observe(_summary(RETURNS))
        out.append(s.plan(_hp(), n_step_max=4))
    return s, out


def test_same_seed_round_and_windows_give_the_same_plan():
    _, a = _plans(3, 3)
    _, b = _plans(3, 3)
    assert a == b and all(len(p) == 4 for p in a)
    _, c = _plans(4, 3)
    assert [[x["dst"] for x in p] for p in c] == [[x["dst"] for x in p] for p in a]  # the ranking is the windows'
    assert c[0] != a[0]  # another seed: other draws
    assert a[0] != a[1]  # another round on the same windows: other draws


def test_explored_values_stay_in_range_and_keep_their_type():
    from evacx.population import per_member
    for seed in range(40):
        s, plans = _plans(seed, 2)
        for d in (x for p in plans for x in p):
            new = d["new"]
            assert sorted(new) == sorted(FULL) == sorted(d["old"])
            assert 1e-6 <= new["lr"] <= 1e-2 and 0.5 <= new["gamma"] <= 0.999
            assert type(new["n_step"]) is int and 1 <= new["n_step"] <= 4  # the ring's cap, below NSTEP_MAX = 32
            assert type(new["target_every"]) is int and new["target_every"] >= 1
            assert new["loss"] in ("mse", "huber") and new["epsilon"] in (0.1, 0.3, 0.9)
            for name, v in new.items():  # what set_hparams will check
                per_member(name, v, 1)
            donor = 1e-3 * (d["src"] + 1)
            assert any(new["lr"] == min(max(donor * f, 1e-6), 1e-2) for f in (0.5, 0.8, 1.25, 2.0))
            _check_map(s, [d])
        _check_map(s, plans[0])
    seen = {x["new"]["target_every"] for seed in range(40) for p in _plans(seed, 1)[1] for x in p}
    assert seen == {1, 5, 20}  # 10 x 0.01 rounds up to 1, never to 0
    s = _sched({"n_step": ("perturb", (100.0,), 1, 1000)}, frac=0.5)
    s.observe(_summary(RETURNS))
    assert all(x["new"]["n_step"] == 32 for x in s.plan(_hp()))  # NSTEP_MAX without a ring's cap


def test_every_plan_map_has_fixed_point_donors():
    for frac in (0.125, 0.25, 0.375, 0.5, 1.0):
        for seed in range(10):
            s = _sched(frac=frac, seed=seed)
            s.observe(_summary([((k * 7 + seed) % 5) * 1.0 for k in range(K)]))
            d = s.plan(_hp())
            assert len(d) == min(int(frac * K), K // 2)
            _check_map(s, d)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("space", [
    {"loss": ("perturb", (0.8, 1.25), 0, 1)}, {"momentum": ("perturb", (0.8,), 0, 1)}, {"lr": ("perturb", (0.8,), 0)},
    {"lr": ("perturb", (), 0, 1)}, {"lr": ("perturb", (0.0, 1.25), 0, 1)}, {"lr": ("perturb", (0.8,), 1e-2, 1e-3)},
    {"lr": ("perturb", (0.8,), -1.0, 1e-3)}, {"gamma": ("perturb", (0.8,), 0.5, 1.5)}, {"lr": ("shake", (0.8,), 0, 1)},
    {"lr": ("resample", ())}, {"lr": ("resample", (1e-3, float("nan")))}, {"loss": ("resample", ("mse", "l1"))},
    {"n_step": ("resample", (1, 2.5))}, {"n_step": ("resample", (1, 33))}, {"lr": "perturb"}, [("lr", SPACE["lr"])],
    {"lr": ("perturb", (float("inf"),), 0, 1)}])
def test_malformed_spaces_are_refused(space):
    with pytest.raises(ValueError):
        _sched(space)


@pytest.mark.parametrize("kw", [dict(members=0), dict(members=65), dict(frac=-0.1), dict(frac=1.5),
                                dict(frac=float("nan")), dict(min_episodes=0), dict(fitness="reward"), dict(seed=-1),
                                dict(people=0)])
def test_bad_scheduler_arguments_are_refused(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        _sched(**kw)


def test_parse_space_reads_the_runner_flag():
    from evacx.pbt import parse_space
    sp = parse_space("lr:perturb:0.8,1.25:1e-6:1e-2; n_step:resample:1,3,5;loss:resample:mse,huber")
    assert sp == {"lr": ("perturb", (0.8, 1.25), 1e-6, 1e-2), "n_step": ("resample", (1, 3, 5)),
                  "loss": ("resample", ("mse", "huber"))}
    for bad in ("lr:perturb:0.8", "lr:resample", "lr:perturb:a,b:0:1", "loss:perturb:0.8:0:1",
                "lr:resample:1e-3;lr:resample:1"):
        with pytest.raises(ValueError):
            parse_space(bad)


def test_runner_flags_need_no_device():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dqn-marl_amd"))
    from Louvre_Evacuation.runners import train_pop
    args = train_pop.parse_args(["--members", "4", "--log-every", "50"])
    assert args.pbt_every == 0 and train_pop.pbt_scheduler(args, 150) is None
    args = train_pop.parse_args(["--members", "4", "--log-every", "50", "--pbt-every", "100", "--pbt-frac", "0.5",
                                 "--pbt-min-episodes", "2", "--pbt-fitness", "evac_rate", "--seed", "3",
                                 "--pbt-space", "lr:perturb:0.8,1.25:1e-6:1e-2;n_step:resample:1,3,5"])
    s = train_pop.pbt_scheduler(args, 150)
    assert (s.K, s.frac, s.min_episodes, s.fitness, s.seed, s.people) == (4, 0.5, 2, "evac_rate", 3, 150)
    assert sorted(s.space) == ["lr", "n_step"]
    for every in ("75", "-50"):
        with pytest.raises(ValueError, match="--pbt-every"):
            train_pop.pbt_scheduler(train_pop.parse_args(["--log-every", "50", "--pbt-every", every]), 150)
    d = dict(dst=3, src=0, fitness_dst=-1.5, fitness_src=2.0, old={"loss": "mse", "lr": 1e-3},
             new={"loss": "huber", "lr": 8e-4})
    assert train_pop.pbt_rows(2, 300, [d], ["loss", "lr"]) == [[2, 300, 3, 0, "-1.5", "2.0", "mse", "huber", "0.001",
                                                                "0.0008"]]


# ------------------------------------------------------------------ evx_copy_members: -22 before any launch
BASE = 0x7000_0000_1000  # never dereferenced


def _copy(bufs, src, members=None, nbufs=None):
    from evacx import _lib
    L = _lib.lib()
    arr = None if bufs is None else (_lib.evx_member_buf * max(1, len(bufs)))(
        *[_lib.evx_member_buf(base=b, stride_bytes=s, bytes=n) for b, s, n in bufs])
    sm = None if src is None else (C.c_int32 * max(1, len(src)))(*src)
    rc = L.evx_copy_members(arr, len(bufs or ()) if nbufs is None else nbufs, sm,
                            len(src or ()) if members is None else members, None)
    return rc, L.evx_last_error().decode()


OK_BUF = (BASE, 64, 64)
REFUSED = {
    "bufs NULL": (dict(bufs=None, src=[0, 0], nbufs=1), "NULL"),
    "src NULL": (dict(bufs=[OK_BUF], src=None, members=2), "NULL"),
    "base NULL": (dict(bufs=[OK_BUF, (0, 64, 64)], src=[0, 0]), "buffer 1 has a NULL base"),
    "members 0": (dict(bufs=[OK_BUF], src=[0], members=0), "members must be 1..64, not 0"),
    "members 65": (dict(bufs=[OK_BUF], src=[0] * 65), "members must be 1..64, not 65"),
    "nbufs 0": (dict(bufs=[OK_BUF], src=[0, 0], nbufs=0), "nbufs must be 1..32, not 0"),
    "nbufs 33": (dict(bufs=[OK_BUF] * 33, src=[0, 0]), "nbufs must be 1..32, not 33"),
    "src negative": (dict(bufs=[OK_BUF], src=[0, -1, 2]), "src[1] = -1"),
    "src too large": (dict(bufs=[OK_BUF], src=[0, 1, 3]), "src[2] = 3"),
    "donor replaced": (dict(bufs=[OK_BUF], src=[0, 0, 1]), "member 2 takes from member 1, which is itself replaced"),
    "swap": (dict(bufs=[OK_BUF], src=[1, 0]), "itself replaced"),
    "bytes odd": (dict(bufs=[(BASE, 64, 62)], src=[0, 0]), "multiples of 4"),
    "stride odd": (dict(bufs=[(BASE, 66, 64)], src=[0, 0]), "multiples of 4"),
    "base unaligned": (dict(bufs=[(BASE + 2, 64, 64)], src=[0, 0]), "multiples of 4"),
    "bytes over stride": (dict(bufs=[(BASE, 64, 68)], src=[0, 0]), "bytes = 68 must lie in 0..stride_bytes = 64"),
    "bytes negative": (dict(bufs=[(BASE, 64, -4)], src=[0, 0]), "bytes = -4"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_copy_members_refuses_before_any_launch(case):
    kw, fragment = REFUSED[case]
    rc, text = _copy(**kw)
    assert rc == -22 and text.startswith("copy_members:") and fragment in text, (rc, text)


def test_copy_members_identity_map_launches_nothing():
    """No device here: a launch would fail, the identity map (and a map of empty blocks) returns 0."""
    assert _copy([OK_BUF, (BASE + 4096, 128, 4)], [0, 1, 2, 3])[0] == 0
    assert _copy([(BASE, 64, 0)], [0, 0])[0] == 0


def test_trainer_map_check_names_the_value():
    from evacx.population import PopulationTrainer

    class _NoDevice(PopulationTrainer):
        def __init__(self, K):
            self.K = K
    t = _NoDevice(4)
    assert t.member_map([0, 0, 2, 2]) == [0, 0, 2, 2] and t.member_map((0, 1, 2, 3)) == [0, 1, 2, 3]
    for bad, what in (([0, 0, 2], "members = 4"), ([0, 0, 2, 4], r"src_map\[3\].*4"),
                      ([0, 0, 1, 3], "member 1 is itself replaced"), ([0, 1.0, 2, 3], r"src_map\[1\].*1\.0"),
                      ([0, True, 2, 3], "True"), (3, "not 3")):
        with pytest.raises(ValueError, match=what):
            t.member_map(bad)
