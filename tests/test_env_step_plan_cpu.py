"""The env step's launch plan (evx_env_step_plan_query, the function step_select itself switches on)
without a GPU: asked at 256 compute units on dummy pointers, as test_env_lds_cpu.py asks for the
LDS bytes. Every case of env_route_cases.py plans as its table entry says, each boundary pair flips
its flag, and the switches of the launcher (envs per CU, EVX_ENV_NWB, the heavy path's conditions)
sit where the header says."""
import ctypes as C

import pytest

from env_route_cases import BOUNDARY_PAIRS, BY_NAME, CASES, HCAP, PLAN_FIELDS
from env_route_util import NCU, assert_plan, case_plan, dummy_layout, dummy_state, plan_query, set_nwb

CFG3 = (128, 128, 2276, 16)   # an ordinary grid
CFG4 = (256, 256, 9102, 1)    # a big grid


def _plan(L, W, P, R, E, order=True, multi=False, ncu=NCU):
    rc, plan, text = plan_query(dummy_layout(L, W, P, R, multi), dummy_state(E, order, multi), ncu)
    assert rc == 0, (rc, text)
    return plan


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_plans_as_the_table_says(case, monkeypatch):
    from evacx import _lib
    set_nwb(monkeypatch, case.flags["nwb"])
    plan = case_plan(case)
    assert_plan(case, plan)
    lay = dummy_layout(case.L, case.W, case.P, case.R)
    assert plan["lds_env_bytes"] == _lib.lib().evx_step_lds_bytes(C.byref(lay))
    per_wg = plan["lds_env_bytes"] * plan["nwb"]
    # 4-wave workgroups of an ordinary grid add the heavy path's control block and, where the rows
    # buffers run past the four env regions, those
    assert plan["lds_wg_bytes"] == per_wg if plan["nwb"] < 4 else plan["lds_wg_bytes"] >= per_wg + 128
    assert (plan["lds_wg_bytes"] > per_wg + 128) == bool(plan["nwb"] == 4 and plan["wide_past_envs"])
    assert plan["lds_wg_bytes"] <= 160 * 1024


@pytest.mark.parametrize("a,b,differ", BOUNDARY_PAIRS, ids=[p[0].split("-")[0] for p in BOUNDARY_PAIRS])
def test_boundary_pair_flips_exactly_its_flag(a, b, differ, monkeypatch):
    set_nwb(monkeypatch, None)
    ca = next(c for c in CASES if c.name.startswith(a) and not c.flags["wide"])
    cb = next(c for c in CASES if c.name.startswith(b) and not c.flags["wide"])
    assert (ca.P, ca.R, ca.E, ca.steps) == (cb.P, cb.R, cb.E, cb.steps)
    pa, pb = case_plan(ca), case_plan(cb)
    assert {k for k in PLAN_FIELDS if pa[k] != pb[k]} == differ
    flag = sorted(differ & {"vac_in_ring", "bigg", "near_in_misc"})
    assert len(flag) == 1 and pa[flag[0]] != pb[flag[0]]


def test_bitmap_words_of_the_boundary_grids():
    """the grids sit on the last and the first size of each branch"""
    def rw(L, W):
        return ((L + 2) * (W + 2) + 31) // 32

    def ncw(L, W):
        return (((L + 2 + 3) >> 2) * ((W + 2 + 3) >> 2) + 31) // 32
    assert (rw(126, 154), rw(106, 183)) == (624, 625)
    assert (rw(179, 179), rw(158, 203)) == (1024, 1025)
    assert (ncw(266, 266), ncw(267, 267)) == (141, 145) and ncw(266, 266) <= 144 < ncw(267, 267)


def test_envs_per_cu_switch_to_one_wave_workgroups(monkeypatch):
    set_nwb(monkeypatch, None)
    for ncu in (NCU, 8):
        assert _plan(*CFG3, E=64 * ncu - 1, ncu=ncu)["nwb"] == 4
        assert _plan(*CFG3, E=64 * ncu, ncu=ncu)["nwb"] == 1
        assert _plan(*CFG4, E=32 * ncu - 1, ncu=ncu)["nwb"] == 2
        assert _plan(*CFG4, E=32 * ncu, ncu=ncu)["nwb"] == 1
    one = _plan(*CFG3, E=64 * NCU)
    assert (one["hcap"], one["hmin"], one["lds_wg_bytes"]) == (0, 0, one["lds_env_bytes"])


def test_nwb_override_is_honoured_and_clamped_on_big_grids(monkeypatch):
    for n in (1, 2, 4):
        set_nwb(monkeypatch, n)
        assert _plan(*CFG3, E=9)["nwb"] == n and _plan(*CFG3, E=64 * NCU)["nwb"] == n
        assert _plan(*CFG4, E=3)["nwb"] == min(n, 2)
        assert _plan(180, 180, 3000, 2, E=3)["nwb"] == min(n, 2)
    for junk in ("3", "0", "8", "x", ""):  # anything else: the default
        monkeypatch.setenv("EVX_ENV_NWB", junk)
        assert _plan(*CFG3, E=9)["nwb"] == 4 and _plan(*CFG4, E=3)["nwb"] == 2
    # the override does not lift the 160 KiB bound
    set_nwb(monkeypatch, 4)
    assert _plan(150, 150, 8000, 2, E=2)["nwb"] == 2


def test_heavy_path_conditions(monkeypatch):
    set_nwb(monkeypatch, None)
    with_order = _plan(*CFG3, E=6)
    assert (with_order["hcap"], with_order["hmin"]) == (HCAP, 2276 // 4)
    assert _plan(4, 4, 1, 1, E=8)["hmin"] == 1  # max(1, P / 4)
    no_order = _plan(*CFG3, E=6, order=False)
    assert (no_order["hcap"], no_order["hmin"], no_order["nwb"]) == (0, 0, 4)
    assert no_order["lds_wg_bytes"] == with_order["lds_wg_bytes"]  # the same workgroup either way
    big = _plan(*CFG4, E=3)
    assert (big["bigg"], big["hcap"], big["hmin"], big["vac_in_ring"], big["wide_past_envs"]) == (1, 0, 0, 0, 0)
    # the 4-wave workgroup of 150x150 with 8000 persons exceeds 160 KiB; with 3000 it fits
    over = _plan(150, 150, 8000, 2, E=2)
    assert (over["nwb"], over["hcap"], over["bigg"], over["wide_past_envs"]) == (2, 0, 0, 1)
    fits = _plan(150, 150, 3000, 2, E=2)
    assert (fits["nwb"], fits["hcap"]) == (4, HCAP)
    for n in (1, 2):
        set_nwb(monkeypatch, n)
        assert _plan(*CFG3, E=6)["hcap"] == 0


def test_multi_needs_the_layout_set_and_the_index(monkeypatch):
    set_nwb(monkeypatch, None)
    assert _plan(*CFG3, E=6, multi=True)["multi"] == 1
    lay, st = dummy_layout(*CFG3, multi=True), dummy_state(6, multi=False)
    assert plan_query(lay, st)[1]["multi"] == 0
    lay, st = dummy_layout(*CFG3, multi=False), dummy_state(6, multi=True)
    assert plan_query(lay, st)[1]["multi"] == 0


def test_argument_errors_are_the_steps_own(monkeypatch):
    from evacx import _lib
    set_nwb(monkeypatch, None)
    st = dummy_state(4)
    ok = dummy_layout(36, 30, 150, 1)
    assert plan_query(None, st)[::2] == (-22, b"layout is NULL")
    assert plan_query(ok, None)[::2] == (-22, b"NULL argument")
    assert _lib.lib().evx_env_step_plan_query(C.byref(ok), C.byref(st), NCU, None) == -22
    assert _lib.lib().evx_last_error() == b"NULL argument"
    for kw, text in [(dict(L=2), b"grid size out of range"), (dict(W=4001), b"grid size out of range"),
                     (dict(P=0), b"P must be in [1, 16383]"), (dict(P=16384), b"P must be in [1, 16383]"),
                     (dict(R=0), b"R must be in [1, 1024]"), (dict(R=1025), b"R must be in [1, 1024]")]:
        lay = dummy_layout(36, 30, 150, 1)
        for k, v in kw.items():
            setattr(lay, k, v)
        assert plan_query(lay, st)[::2] == (-22, text), kw
    lay = _lib.evx_layout(L=36, W=30, P=150, R=1)
    assert plan_query(lay, st)[::2] == (-22, b"missing table")
    # the step's own texts for sizes past its keys and past the LDS
    assert plan_query(dummy_layout(4000, 4000, 16383, 1), st)[::2] == \
        (-22, b"grid cells x people too large for 32-bit move keys")
    assert plan_query(dummy_layout(2000, 2000, 100, 1), st)[::2] == (-7, b"layout needs more than 160 KiB of LDS")
    # and the same call with the same arguments through the step itself (no device is touched
    # before these checks)
    out = _lib.evx_step_out(reward=8, done=8, obs=8)
    stp = _lib.evx_state(E=4, scratch=8)
    for lay in (dummy_layout(4000, 4000, 16383, 1), dummy_layout(36, 30, 0, 1)):
        lay.nbr_valid = lay.floor_d5 = 8
        rc = _lib.lib().evx_env_step(C.byref(lay), C.byref(stp), 8, C.byref(out), None)
        text = _lib.lib().evx_last_error()
        assert (rc, text) == plan_query(lay, st)[::2]


def _trajectory(c):
    """what the oracle's side of a case depends on (the dispatch flavours share a trajectory)"""
    f = c.flags
    return (c.L, c.W, c.R, c.P, c.E, c.steps, f["layouts"], f["jump"], f["reset"], f["floor"], f["heavy"])


SMALL_TRAJECTORIES = list({_trajectory(c): c for c in CASES if (c.L + 2) * (c.W + 2) <= 2048}.values())


@pytest.mark.parametrize("case", SMALL_TRAJECTORIES, ids=[c.name for c in SMALL_TRAJECTORIES])
def test_small_cases_meet_their_coverage_conditions_in_the_oracle(case):
    """The conditions of the GPU cases (an evacuation, a death, an episode end, a person within a
    robot's range, every env heavy at once) depend on the oracle alone: the small grids' are
    checked here too, so a seed or a step count that makes a case vacuous shows without a GPU."""
    from env_route_util import run_case
    fig = run_case(case, device=False)
    assert fig["checks"] == case.steps // case.every + 1


def test_env_lds_bytes_of_known_layouts(monkeypatch):
    """the plan's per-env bytes are evx_step_lds_bytes' (test_env_lds_cpu.py pins those)"""
    set_nwb(monkeypatch, None)
    assert _plan(*CFG3, E=6)["lds_env_bytes"] == 12800
    assert _plan(178, 178, 1500, 2, E=2)["lds_env_bytes"] == 21056
    assert BY_NAME["small-nwb4"].plan["hcap"] == HCAP
