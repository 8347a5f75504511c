"""Episode statistics without a GPU: the C entry points refuse NULL buffers with a message and
touch no device; the Python front ends check their arguments before any launch."""
import ctypes

import pytest
import torch


def _loaded():
    from evacx import _lib
    return _lib.lib()


def _host_descriptor(E=4, leave_out=None):
    """An evx_episodes whose pointers are (host) scratch: only ever passed to calls that must fail
    before they launch anything."""
    from evacx.episodes import evx_episodes
    keep = []
    d = evx_episodes(E=E, tab_slots=0)
    for name, _ in evx_episodes._fields_[2:17]:
        if name == leave_out:
            continue
        buf = (ctypes.c_int64 * E)()
        keep.append(buf)
        setattr(d, name, ctypes.addressof(buf))
    return d, keep


def test_update_refuses_null_buffers():
    L = _loaded()
    assert L.evx_episode_update(None, None, None, None, 0, None) < 0
    assert b"NULL episode descriptor" in L.evx_episode_last_error()
    d, keep = _host_descriptor(leave_out="w_ret2")
    assert L.evx_episode_update(ctypes.byref(d), None, None, None, 0, None) < 0
    assert b"episode_update" in L.evx_episode_last_error() and b"NULL episode buffer" in L.evx_episode_last_error()
    d, keep = _host_descriptor()
    assert L.evx_episode_update(ctypes.byref(d), None, None, None, 0, None) < 0
    assert b"NULL reward, done or counts" in L.evx_episode_last_error()
    d.E = 0
    assert L.evx_episode_update(ctypes.byref(d), None, None, None, 0, None) < 0
    assert b"E must be >= 1" in L.evx_episode_last_error()
    d.E, d.tab_slots = 4, 2  # a table without its buffers
    assert L.evx_episode_update(ctypes.byref(d), None, None, None, 0, None) < 0
    assert b"table" in L.evx_episode_last_error()


def test_discard_and_init_refuse_null_buffers():
    L = _loaded()
    assert L.evx_episode_discard(None, None, None) < 0
    assert b"episode_discard" in L.evx_episode_last_error()
    d, keep = _host_descriptor(leave_out="len")
    assert L.evx_episode_discard(ctypes.byref(d), None, None) < 0
    assert b"NULL episode buffer" in L.evx_episode_last_error()
    assert L.evx_episode_init(ctypes.byref(d), None) < 0
    assert b"episode_init" in L.evx_episode_last_error()


def test_reduce_refuses_null_buffers_and_bad_layout_counts():
    L = _loaded()
    assert L.evx_episode_reduce(None, None, 1, 0, None, 0, None) < 0
    assert b"episode_reduce" in L.evx_episode_last_error()
    d, keep = _host_descriptor(leave_out="n_total")
    rows = (ctypes.c_int64 * 40)()
    assert L.evx_episode_reduce(ctypes.byref(d), None, 1, 0, rows, 0, None) < 0
    assert b"NULL episode buffer" in L.evx_episode_last_error()
    d, keep = _host_descriptor()
    assert L.evx_episode_reduce(ctypes.byref(d), None, 1, 0, None, 0, None) < 0
    assert b"NULL output rows" in L.evx_episode_last_error()
    assert L.evx_episode_reduce(ctypes.byref(d), None, 0, 0, rows, 0, None) < 0
    assert b"n_layouts" in L.evx_episode_last_error()
    assert L.evx_episode_reduce(ctypes.byref(d), None, 3, 0, rows, 0, None) < 0
    assert b"layout_idx" in L.evx_episode_last_error()


def test_descriptor_mirrors_the_header():
    """The ctypes structures have the C sizes (pointers after two int32; 10 words per row)."""
    from evacx import episodes
    assert ctypes.sizeof(episodes.evx_episodes) == 8 + 19 * ctypes.sizeof(ctypes.c_void_p)
    assert episodes.ROW_WORDS == 10
    import os
    import re
    from golden_util import ROOT
    src = open(os.path.join(ROOT, "include", "evacx.h")).read()
    assert int(re.search(r"#define EVX_EPISODE_REDUCE_SPAN (\d+)", src).group(1)) == episodes.REDUCE_SPAN


def test_episode_stats_argument_checks_need_no_device():
    from evacx.episodes import EpisodeStats
    with pytest.raises(ValueError):
        EpisodeStats(0, "cuda", 150)
    with pytest.raises(ValueError):
        EpisodeStats(8, "cuda", 0)
    with pytest.raises(ValueError):
        EpisodeStats(8, "cuda", 150, cap=-1)
    with pytest.raises(ValueError):
        EpisodeStats(8, "cuda", 150, n_layouts=0)
    with pytest.raises(ValueError):
        EpisodeStats(8, "cuda", 150, n_layouts=2)  # several layouts, no layout_idx
    with pytest.raises(ValueError):
        EpisodeStats(8, "cuda", 150, layout_idx=torch.zeros(7, dtype=torch.int32), n_layouts=2)  # size
    with pytest.raises(ValueError):
        EpisodeStats(8, "cuda", 150, layout_idx=torch.zeros(8, dtype=torch.int64), n_layouts=2)  # dtype
    with pytest.raises(ValueError):
        EpisodeStats(8, "cuda", 150, layout_idx=torch.zeros(8, dtype=torch.int32), n_layouts=2)  # not on the device


def test_summary_row_without_episodes_has_none_not_nan():
    from evacx.episodes import _row_dict
    inf = float("inf")
    d = _row_dict([0, 0, 0, 0, 0, 0, 0, 0, 5, 5], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, inf, -inf, 0.0, 0.0], 150)
    assert d["episodes"] == 0 and d["remaining"] == 5
    for k in ("return_mean", "return_std", "return_min", "return_max", "length_mean", "evac_rate", "death_rate"):
        assert d[k] is None, k
    d = _row_dict([2, 90, 250, 50, 0, 0, 0, 0, 0, 0], [0.0, 0.0, 0.0, 0.0, 10.0, 58.0, 3.0, 7.0, 0.0, 0.0], 150)
    assert d["return_mean"] == 5.0 and d["return_std"] == 2.0 and d["length_mean"] == 45.0
    assert d["evac_rate"] == 250 / 300 and d["death_rate"] == 50 / 300
    assert (d["return_min"], d["return_max"]) == (3.0, 7.0)


def test_evaluate_rejects_unknown_policies_before_the_device():
    from evacx.evaluate import evaluate
    for bad in ("bogus", 5, -1, None, 1.5, True):
        with pytest.raises(ValueError):
            evaluate(None, 8, 2, bad)
    with pytest.raises(ValueError):
        evaluate(None, 8, 2, "greedy")  # no learner
    with pytest.raises(ValueError):
        evaluate(None, 0, 2, 1)


def test_runner_arguments():
    from Louvre_Evacuation.runners import train_vec
    a = train_vec.parse_args(["--envs", "64", "--steps", "60", "--log-every", "20", "--qnet", "conv", "--out", "x",
                              "--eval-episodes", "2"])
    assert (a.envs, a.steps, a.log_every, a.qnet, a.out, a.eval_episodes) == (64, 60, 20, "conv", "x", 2)
    assert a.config.endswith("dqn.yaml")
    assert train_vec.CSV_COLUMNS == ["step", "episodes", "reward", "evac_rate", "death_rate", "length", "loss",
                                     "epsilon"]
