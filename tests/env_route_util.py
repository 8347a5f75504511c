"""Shared by test_env_step_plan_cpu.py and test_env_routes_gpu.py: the plan query on dummy pointers,
the layouts of a case of env_route_cases.py, and the runner that steps a case on the GPU and in the
C oracle with the same seeds and actions and compares them bit for bit (a generalisation of
test_env_gpu._oracle_pair: LayoutSets, the age jump to the time limit, both reset flavours, the
forced heavy-first order in one or two launches, the EVX_ENV_NWB override)."""
import ctypes as C
import dataclasses
import functools

import numpy as np

from env_route_cases import PLAN_FIELDS

NCU = 256  # the compute units the case table's plans are stated for (an MI355X has 256)
SEED0, ACT_SEED = 1234, 7
JUMP_TO = 1190  # current_step after the age jump: time = 0.5 * current_step reaches 600 ten steps on
STATE_FIELDS = ["pos", "health", "acc", "flags", "rmap", "robots", "view", "scal", "py_mt", "np_mt"]


# ---------------------------------------------------------------------------------- the plan
def dummy_layout(L, W, P, R, multi=False):
    """An evx_layout with sizes only: the plan and size queries read no table (any non-NULL value)."""
    from evacx import _lib
    lay = _lib.evx_layout(L=L, W=W, P=P, R=R)
    for k in ["floor", "cellinfo", "valid_bits", "danger_p", "danger_o"]:
        setattr(lay, k, 8)
    if multi:
        lay.layout_set = 8
    return lay


def dummy_state(E, order=True, multi=False):
    from evacx import _lib
    return _lib.evx_state(E=E, order=8 if order else None, layout_idx=8 if multi else None)


def plan_query(lay, st, ncu=NCU):
    """(rc, plan as a dict, error text) of evx_env_step_plan_query"""
    from evacx import _lib
    p = _lib.evx_env_step_plan()
    rc = _lib.lib().evx_env_step_plan_query(C.byref(lay) if lay is not None else None,
                                            C.byref(st) if st is not None else None, ncu, C.byref(p))
    return rc, {n: getattr(p, n) for n, _ in p._fields_}, _lib.lib().evx_last_error()


def case_plan(case, ncu=NCU, E=None, order=True):
    """The plan of a case's sizes on dummy pointers (the caller sets EVX_ENV_NWB)."""
    multi = case.flags["layouts"] > 0
    rc, plan, text = plan_query(dummy_layout(case.L, case.W, case.P, case.R, multi),
                                dummy_state(case.E if E is None else E, order, multi), ncu)
    assert rc == 0, (case.name, rc, text)
    return plan


def set_nwb(monkeypatch, nwb):
    """EVX_ENV_NWB for the launcher and the queries, which read it on every call."""
    if nwb is None:
        monkeypatch.delenv("EVX_ENV_NWB", raising=False)
    else:
        monkeypatch.setenv("EVX_ENV_NWB", str(nwb))


def assert_plan(case, plan):
    got = {k: plan[k] for k in PLAN_FIELDS}
    assert got == case.plan, (case.name, got, case.plan)


# ---------------------------------------------------------------------------------- layouts
def layout_specs(L, W, R, floor=None, layouts=0):
    """The LayoutSpecs of a case: one (layouts = 0), or the n of its LayoutSet -- the base layout and
    variants with other barriers, exit and fire sources (test_layoutset_gpu._specs, scaled to the
    grid). floor: None for synthetic(L, W, R), else random_layout's seed."""
    from evacx.layout import random_layout, synthetic
    s0 = synthetic(L, W, R) if floor is None else random_layout(L, W, R, floor)
    if not layouts:
        return [s0]
    sx, sy = L / 24.0, W / 20.0

    def pt(x, y):
        return (int(round(x * sx)), int(round(y * sy)))
    s1 = dataclasses.replace(s0, barriers=((pt(5, 5), pt(8, 9)),), exit=(L, pt(0, 3)[1]))
    s2 = dataclasses.replace(s0, barriers=((pt(3, 10), pt(6, 15)), (pt(21, 2), pt(22, 6))), exit=(pt(10, 0)[0], W),
                             additional_fire=())
    specs = [s0, s1, s2][:layouts]
    assert len(specs) == layouts
    for s in specs:  # no robot starts inside a barrier
        for (a, b) in s.barriers:
            assert not any(a[0] <= x <= b[0] and a[1] <= y <= b[1] for (x, y) in s.robot_init), s.barriers
    return specs


@functools.lru_cache(maxsize=3)
def _tables(L, W, R, floor, layouts):
    from evacx.layout import build_tables
    return [build_tables(s) for s in layout_specs(L, W, R, floor, layouts)]


def case_tables(case):
    """LayoutTables of the case's layouts, shared by the cases of one size (read-only)."""
    return _tables(case.L, case.W, case.R, case.flags["floor"], case.flags["layouts"])


def layout_of(case):
    n = case.flags["layouts"]
    return [(7 * i) % n for i in range(case.E)] if n else [0] * case.E


# ---------------------------------------------------------------------------------- the runner
def _near_robot(oe, repel_range=5.0):
    """a person in play (not safe, not dead) within the repel range of a robot"""
    pos = oe.pos[oe.flags == 0].astype(np.int64)
    if not len(pos):
        return False
    d = pos[:, None, :] - oe.robots.astype(np.int64)[None, :, :]
    return bool(((d * d).sum(-1) < repel_range * repel_range).any())


def run_case(case, monkeypatch=None, device=True):
    """Step the case's E envs on the GPU (device=True) and in the oracle, compare, and check the
    case's coverage conditions on the oracle's states. device=False runs the oracle alone (the
    conditions without a GPU). Returns the figures of the run."""
    from oracle import oracle as orc
    f = case.flags
    P, R, E = case.P, case.R, case.E
    tabs = case_tables(case)
    lof = layout_of(case)
    olays = [orc.Layout.from_tables(t, P) for t in tabs]
    oenvs = [orc.Env(olays[lof[i]], thmap=f["thmap"]) for i in range(E)]
    for i, oe in enumerate(oenvs):
        oe.seed(SEED0 + i)
    env = None
    if device:
        import torch
        from evacx import _lib
        from evacx.env import DeviceLayout, LayoutSet, VecEnv
        set_nwb(monkeypatch, f["nwb"])
        dl = [DeviceLayout(t, P) for t in tabs]
        if f["layouts"]:
            lay = LayoutSet(dl)
            env = VecEnv(lay, E, thmap=f["thmap"], layout_of=lof)
        else:
            lay = dl[0]
            env = VecEnv(lay, E, thmap=f["thmap"])
        # the route: the launcher's own plan for this very layout and state on this device, at the
        # table's 256 compute units, and the workgroup the occupancy query reports
        for ncu in (0, NCU):
            rc, plan, text = plan_query(lay.c, env.c, ncu)
            assert rc == 0, (rc, text)
            assert_plan(case, plan)
        n, lds, thr = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().evx_env_step_occupancy(C.byref(lay.c), C.byref(env.c), C.byref(n), C.byref(lds),
                                                     C.byref(thr)), "evx_env_step_occupancy")
        assert thr.value == 64 * case.plan["nwb"] and lds.value == plan["lds_wg_bytes"] and n.value >= 1
        assert plan["lds_env_bytes"] == _lib.lib().evx_step_lds_bytes(C.byref(lay.c))
        env.seed([SEED0 + i for i in range(E)])
        env.reset()
    oobs = [oe.reset() for oe in oenvs]
    rng = np.random.RandomState(ACT_SEED)
    fig = dict(resets=0, evac=0, dead=0, near=False, max_heavy=0, checks=0)
    hmin, hcap = case.plan["hmin"], case.plan["hcap"]
    auto = f["reset"] == "fused"

    def compare(s):
        fig["checks"] += 1
        fig["near"] = fig["near"] or any(_near_robot(oe) for oe in oenvs)
        if not device:
            return
        obs64 = env.expand_obs(torch.float64).cpu().numpy()
        obs32 = env.expand_obs(torch.float32).cpu().numpy()
        sts = env.host_states(range(E))
        for i in range(E):
            ost = oenvs[i].state()
            for name in STATE_FIELDS:
                assert np.array_equal(sts[i][name], ost[name]), (s, i, name)
            if f["thmap"]:
                assert np.array_equal(sts[i]["thmap"], ost["thmap"]), (s, i, "thmap")
            assert np.array_equal(obs64[i], oobs[i]), (s, i, "obs")
            assert np.array_equal(obs32[i], oobs[i].astype(np.float32)), (s, i, "obs32")

    for s in range(case.steps + 1):
        if s > 0:
            acts = rng.randint(0, 5, size=(E, R)).astype(np.int32)
            acts[rng.rand(E, R) < 0.02] = 7  # invalid actions are ignored by the reference
            # the envs the heavy-first order must list as heavy: the oracle's persons in play
            heavy_want = min(hcap, sum(int(P - oe.scal[2] - oe.scal[3] >= hmin) for oe in oenvs))
            if device:
                a = torch.from_numpy(acts.reshape(-1)).cuda()
                if f["wide"]:
                    env.compute_order(force=True)
                    if f["heavy"]:
                        heavy = int(env.order[E].item())
                        assert heavy == heavy_want, (s, heavy, heavy_want)
                        fig["max_heavy"] = max(fig["max_heavy"], heavy)
                if f["parts"]:
                    env.step(a, order=False, auto_reset=auto, part=1)
                    env.step(a, order=False, auto_reset=auto, part=2)
                else:
                    env.step(a, order=not f["wide"], auto_reset=auto)
            elif f["heavy"]:
                fig["max_heavy"] = max(fig["max_heavy"], heavy_want)
            res = [oe.step(acts[i]) for i, oe in enumerate(oenvs)]
            oobs = [r[0] for r in res]
            odone = np.array([r[2] for r in res], bool)
            fig["evac"] = max(fig["evac"], max(int(oe.scal[2]) for oe in oenvs))
            fig["dead"] = max(fig["dead"], max(int(oe.scal[3]) for oe in oenvs))
            if device:
                rew = env.reward.cpu().numpy()
                done = env.done.cpu().numpy().astype(bool)
                for i in range(E):
                    assert rew[i] == res[i][1], (s, i, rew[i], res[i][1])
                    assert done[i] == res[i][2], (s, i)
                if auto and odone.any():
                    term = env.expand_obs(torch.float64, env.obs_term).cpu().numpy()
                    for i in np.nonzero(odone)[0]:
                        assert np.array_equal(term[i], oobs[i]), (s, i, "terminal obs")
            if auto:
                for i in np.nonzero(odone)[0]:
                    oobs[i] = oenvs[i].reset()
                    fig["resets"] += 1
        if s % case.every == 0 or s == case.steps:
            compare(s)
        if s > 0 and not auto and odone.any():
            if device:
                env.reset(mask=torch.from_numpy(odone).cuda())
            for i in np.nonzero(odone)[0]:
                oobs[i] = oenvs[i].reset()
                fig["resets"] += 1
        if s == f["jump"]:
            if device:  # the device's own state goes back into the oracle: both sides age together
                env.scal.view(E, 4)[:, 1] = JUMP_TO
                env.refresh_classes()
                for oe, st in zip(oenvs, env.host_states(range(E))):
                    oe.load_state(st)
            else:
                for oe in oenvs:
                    oe.scal[1] = JUMP_TO
                    oe.time[0] = 0.5 * JUMP_TO
    if device:
        env.check_err()
    # coverage conditions, from the oracle's states alone
    need = f["need"]
    assert "evac" not in need or fig["evac"] >= 1, (case.name, "nobody evacuated", fig)
    assert "death" not in need or fig["dead"] >= 1, (case.name, "nobody died", fig)
    assert "end" not in need or fig["resets"] >= 1, (case.name, "no episode ended", fig)
    assert "near" not in need or fig["near"], (case.name, "nobody came within a robot's repel range", fig)
    if f["heavy"]:
        assert fig["max_heavy"] == min(hcap, E), (case.name, "not every env was heavy at once", fig)
    return fig
