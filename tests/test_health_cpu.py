"""Terminal health without a GPU: numpy's summation order of np.mean restated (the order
csrc/health.hip implements), the library's evx_health_* symbols, and the entry points' refusals,
which touch no device."""
import ctypes

import numpy as np
import pytest

import health_util as hu


@pytest.mark.parametrize("n", hu.SIZES)
def test_chunked_pairwise_rule_equals_np_mean(n):
    a = hu.healths(n)
    want = np.mean(a)
    got = hu.chunked_mean(a)
    assert hu.bits(got) == hu.bits(want), (n, got, want)
    assert hu.bits(np.mean(list(a))) == hu.bits(want)  # a list, as the reference passes


@pytest.mark.parametrize("n", [8193, 9102])
def test_plain_pairwise_differs_past_one_chunk(n):
    """The inputs of the GPU test at these sizes tell the two orders apart: plain pairwise over
    the whole list (the oracle's sum, env_step's reward order) is not np.mean's value."""
    from oracle import oracle as orc
    a = hu.healths(n)
    plain = orc.pairwise_sum(a) / n
    assert hu.bits(orc.pairwise_sum(a)) == hu.bits(hu.pairwise(list(a)))  # the restated tree is the oracle's
    assert hu.bits(plain) != hu.bits(np.mean(a)), n
    assert hu.bits(hu.chunked_mean(a)) == hu.bits(np.mean(a)), n


def test_empty_list_is_nan():
    assert np.isnan(hu.chunked_mean([]))


def test_library_exports_the_health_entries():
    from evacx import _lib
    L = _lib.lib()
    names = ["evx_health_init", "evx_health_update", "evx_health_reduce", "evx_health_last_error"]
    for s in names:
        assert hasattr(L, s), s
        assert s in _lib.SIGNATURES, s


def _host_descriptor(E=4, leave_out=None):
    """An evx_health whose pointers are (host) scratch: only ever passed to calls that must fail
    before they launch anything."""
    from evacx.health import evx_health
    keep = []
    d = evx_health(E=E, tab_slots=0)
    for name, _ in evx_health._fields_[2:12]:
        if name == leave_out:
            continue
        buf = (ctypes.c_int64 * E)()
        keep.append(buf)
        setattr(d, name, ctypes.addressof(buf))
    return d, keep


def test_entries_refuse_null_pointers_and_sizes_out_of_range():
    from evacx import _lib
    L = _lib.lib()
    err = L.evx_health_last_error
    pk, hl, dn = (ctypes.c_int64 * 64)(), (ctypes.c_int64 * 64)(), (ctypes.c_int64 * 8)()
    assert L.evx_health_update(None, pk, hl, 4, dn, 0, None) == -22
    assert b"NULL health descriptor" in err()
    d, keep = _host_descriptor(leave_out="w_avg")
    assert L.evx_health_update(ctypes.byref(d), pk, hl, 4, dn, 0, None) == -22
    assert b"health_update" in err() and b"NULL health buffer" in err()
    assert L.evx_health_init(ctypes.byref(d), None) == -22 and b"health_init" in err()
    d, keep = _host_descriptor()
    for args in ((None, hl, dn), (pk, None, dn), (pk, hl, None)):
        assert L.evx_health_update(ctypes.byref(d), args[0], args[1], 4, args[2], 0, None) == -22
        assert b"NULL pk, health or done" in err()
    for P in (0, -1, 16384, 1 << 20):
        assert L.evx_health_update(ctypes.byref(d), pk, hl, P, dn, 0, None) == -22, P
        assert b"P must be 1..16383" in err()
    d.E = 0
    assert L.evx_health_update(ctypes.byref(d), pk, hl, 4, dn, 0, None) == -22 and b"E must be >= 1" in err()
    d.E, d.tab_slots = 4, 2  # a table without its buffers
    assert L.evx_health_update(ctypes.byref(d), pk, hl, 4, dn, 0, None) == -22 and b"table" in err()
    d, keep = _host_descriptor()
    rows = (ctypes.c_int64 * 24)()
    assert L.evx_health_reduce(None, None, 1, rows, 0, None) == -22 and b"health_reduce" in err()
    assert L.evx_health_reduce(ctypes.byref(d), None, 1, None, 0, None) == -22 and b"NULL output rows" in err()
    assert L.evx_health_reduce(ctypes.byref(d), None, 0, rows, 0, None) == -22 and b"n_layouts" in err()
    assert L.evx_health_reduce(ctypes.byref(d), None, 3, rows, 0, None) == -22 and b"layout_idx" in err()


def test_descriptor_mirrors_the_header():
    import os
    import re
    from golden_util import ROOT
    from evacx import health
    assert ctypes.sizeof(health.evx_health) == 8 + 13 * ctypes.sizeof(ctypes.c_void_p)
    src = open(os.path.join(ROOT, "include", "evacx.h")).read()
    assert int(re.search(r"#define EVX_HEALTH_MAX_P (\d+)", src).group(1)) == health.MAX_P == 16383
    row = re.search(r"typedef struct \{([^}]*)\} evx_health_row;", src).group(1)
    assert len(re.findall(r"\b[a-z_]+(?=[,;])", row)) == health.ROW_WORDS


def test_front_ends_check_their_arguments_before_the_device():
    import torch
    from evacx.evaluate import evaluate
    from evacx.health import HealthStats
    for bad in (dict(E=0, P=150), dict(E=8, P=0), dict(E=8, P=16384), dict(E=8, P=150, cap=-1),
                dict(E=8, P=150, n_layouts=0), dict(E=8, P=150, n_layouts=2),
                dict(E=8, P=150, n_layouts=2, layout_idx=torch.zeros(7, dtype=torch.int32))):
        with pytest.raises(ValueError):
            HealthStats(bad.pop("E"), "cuda", bad.pop("P"), **bad)
    with pytest.raises(ValueError):
        evaluate(None, 8, 2, "greedy", metrics=True)  # no learner


def test_summary_row_without_episodes_has_none_not_nan():
    from evacx.health import _row_dict
    inf = float("inf")
    d = _row_dict([0, 0, 0, 0, 0, 0], [0.0, 0.0, 0.0, 0.0, 0.0, inf])
    for k in ("avg_health", "min_health_mean", "min_health", "alive_mean"):
        assert d[k] is None, k
    d = _row_dict([4, 3, 20, 0, 0, 0], [0.0, 0.0, 0.0, 150.0, 260.0, 20.0])  # one episode with nobody alive
    assert d["avg_health"] == 50.0 and d["min_health_mean"] == 65.0 and d["min_health"] == 20.0
    assert d["alive_mean"] == 5.0 and d["episodes"] == 4 and d["health_episodes"] == 3


def test_grouped_load_state_dict_refuses_before_writing():
    """The shape checks of GroupedLearner.load_state_dict run on the dict alone."""
    import torch
    from evacx.qgroup import GroupedLearner
    from golden_util import mlp_shapes
    g = GroupedLearner.__new__(GroupedLearner)
    g.G, g.shapes = 2, mlp_shapes()
    sd = {k: torch.zeros(s) for k, s in mlp_shapes().items()}
    with pytest.raises(ValueError, match="g must be"):
        g.load_state_dict(2, sd)
    bad = dict(sd)
    bad["fc2.weight"] = torch.zeros(256, 511)
    with pytest.raises(ValueError, match="fc2.weight"):
        g.load_state_dict(0, bad)
    bad = {k: v for k, v in sd.items() if k != "fc3.bias"}
    with pytest.raises(ValueError, match="fc3.bias"):
        g.load_state_dict(0, bad)
    bad = dict(sd, **{"conv1.weight": torch.zeros(32, 6, 3, 3)})
    with pytest.raises(ValueError, match="conv1.weight"):
        g.load_state_dict(0, bad)


def test_runner_arguments():
    from Louvre_Evacuation.runners import evaluate_vec
    a = evaluate_vec.parse_args(["--envs", "8", "--robots", "2", "--episodes", "3", "--per-robot", "a.pth", "b.pth",
                                 "--out", "x"])
    assert (a.envs, a.robots, a.episodes, a.per_robot, a.out, a.dqn, a.qmix) == (8, 2, 3, ["a.pth", "b.pth"], "x",
                                                                                 None, None)
    assert evaluate_vec.CSV_COLUMNS == ["strategy", "avg_health", "death_rate", "evac_rate", "avg_time", "episodes"]
    help_text = " ".join(evaluate_vec.build_parser().format_help().split())
    assert "no robot" in help_text.lower() and "(1000, 1000)" in help_text  # the strategy left out, and why
    spec = evaluate_vec.build_spec(dict(width=36, height=30, exit_location=[36, 15]), 2)
    assert spec.R == 2 and spec.reset_robots
    with pytest.raises(ValueError):
        evaluate_vec.strategies(a, 3, "cpu")  # two checkpoints for three robots, before any is read
