"""Evacuation timelines without a GPU: the update restated in numpy (timeline_util.timeline_ref)
against the reference's own trajectories through the host half of Timeline.curves(), the entry
points' refusals (which touch no device), the front ends' argument checks, and the figure."""
import ctypes
import os

import numpy as np
import pytest

import timeline_util as tu

TRAJS = ["cfg1_single_traj", "cfg1_multi_traj"]
P = 150


def _episode_curves(name, a, b, T=96):
    """One fixture episode (reset row a, rows a + 1 .. b its steps) alone: E = 1, cap = 0."""
    from evacx.timeline import build_curves
    tr, pk, _ = tu.fixture(name)
    ref = tu.timeline_ref(1, P, T, track=([0] * P, list(range(P))))
    ref.trace0(pk[a], tr["snap_health"][a])
    for k in range(a + 1, b + 1):
        assert tr["cur_step"][k] == ref.t[0] + 1
        ref.update([[tr["evac"][k], tr["dead"][k]]], [tr["done"][k]], pk[k], tr["snap_health"][k])
    trace = dict(env=ref.trk_env, person=ref.trk_person, pk=ref.trk_pk, health=ref.trk_health, len=ref.trk_len)
    return ref, build_curves({k: getattr(ref, k) for k in tu.SLOTS}, ref.late, int(ref.bad_health[0]), P, trace)


@pytest.mark.parametrize("name", TRAJS)
def test_curves_give_back_the_fixture_counts_at_every_step(name):
    tr, pk, eps = tu.fixture(name)
    assert len(eps) >= 2
    for a, b in eps:
        n = b - a
        ref, cv = _episode_curves(name, a, b)
        assert cv["episodes"] == 1 and cv["bad_health"] == 0 and not cv["late"].any()
        assert np.array_equal(cv["step"][:n], tr["cur_step"][a + 1:b + 1])
        assert np.array_equal(cv["time_s"][:n], tr["time"][a + 1:b + 1])
        # the cumulative curves are the fixture's own counts, exactly; afterwards they stay
        assert np.array_equal(cv["evacuated_mean"][:n], tr["evac"][a + 1:b + 1].astype(np.float64))
        assert np.array_equal(cv["dead_mean"][:n], tr["dead"][a + 1:b + 1].astype(np.float64))
        assert (cv["evacuated_mean"][n:] == tr["evac"][b]).all() and (cv["dead_mean"][n:] == tr["dead"][b]).all()
        assert np.array_equal(cv["remaining_mean"][:n], (P - tr["evac"] - tr["dead"])[a + 1:b + 1].astype(np.float64))
        assert np.array_equal(cv["new_evacuated"][:n], np.diff(tr["evac"][a:b + 1]))
        assert np.array_equal(cv["new_dead"][:n], np.diff(tr["dead"][a:b + 1]))
        assert cv["running"][:n].tolist() == [1] * n and not cv["running"][n:].any()
        assert cv["ended"].sum() == 1 and cv["ended"][n - 1] == 1
        assert cv["per_layout"][0]["new_evacuated"].tolist() == cv["new_evacuated"].tolist()
        assert ref.n_total[0] == 1 and ref.t[0] == 0


@pytest.mark.parametrize("name", TRAJS)
def test_avg_health_is_np_mean_within_the_half_unit_rounding(name):
    """Every person's health is rounded to 2^-20 units, half a unit at most each, so the mean moves by
    at most 2^-21; 1e-9 covers the float64 arithmetic of both means."""
    tr, pk, eps = tu.fixture(name)
    assert tr["snap_health"].min() >= 0.0 and tr["snap_health"].max() <= 100.0  # the overflow bound's premise
    worst = 0.0
    for a, b in eps:
        _, cv = _episode_curves(name, a, b)
        for s, k in enumerate(range(a + 1, b + 1)):
            want = tu.mean_not_dead(tr["snap_flags"][k], tr["snap_health"][k])
            got = cv["avg_health"][s]
            if np.isnan(want):
                assert np.isnan(got), (k, got)
                continue
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 2.0 ** -21 + 1e-9, (k, got, want)
            assert cv["alive"][s] == int(((tr["snap_flags"][k] & 2) == 0).sum())
        assert np.isnan(cv["avg_health"][b - a:]).all()  # nobody is counted after the end
    print(f"{name}: worst |avg_health - np.mean| = {worst:.3e}")


@pytest.mark.parametrize("name", TRAJS)
def test_decoded_trace_is_the_fixture_snapshot(name):
    tr, pk, eps = tu.fixture(name)
    a, b = eps[0]
    _, cv = _episode_curves(name, a, b)
    t = cv["tracked"]
    n = b - a + 1
    assert (t["len"] == n).all() and t["person"].tolist() == list(range(P))
    assert np.array_equal(t["x"][:n], tr["snap_pos"][a:b + 1, :, 0]) and np.array_equal(t["y"][:n],
                                                                                      tr["snap_pos"][a:b + 1, :, 1])
    assert np.array_equal(t["safe"][:n], (tr["snap_flags"][a:b + 1] & 1) != 0)
    assert np.array_equal(t["dead"][:n], (tr["snap_flags"][a:b + 1] & 2) != 0)
    assert np.array_equal(t["health"][:n].view(np.int64), tr["snap_health"][a:b + 1].view(np.int64))
    for i in range(P):
        for key, bit in (("evac_step", 1), ("death_step", 2)):
            on = np.nonzero(tr["snap_flags"][a:b + 1, i] & bit)[0]
            assert t[key][i] == (on[0] if len(on) else -1), (i, key)
    assert (t["evac_step"] >= 0).sum() == tr["evac"][b] and (t["death_step"] >= 0).sum() == tr["dead"][b]


def test_rows_add_up_and_late_steps_are_counted():
    from evacx.timeline import build_curves
    rng = np.random.default_rng(3)
    E, Pn, T = 5, 7, 4
    ref = tu.timeline_ref(E, Pn, T, n_rows=2, layout_idx=[0, 1, 1, 0, 1], cap=1)
    ev, dd = np.zeros(E, np.int64), np.zeros(E, np.int64)
    for step in range(7):
        ev += rng.integers(0, 2, E)
        done = np.full(E, step == 6, np.uint8)
        health = rng.random((E, Pn)) * 100
        ref.update(np.stack([ev, dd], 1), done, np.zeros((E, Pn), np.uint32), health)
    cv = build_curves({k: getattr(ref, k) for k in tu.SLOTS}, ref.late, 0, Pn)
    assert cv["episodes"] == E and [r["episodes"] for r in cv["per_layout"]] == [2, 3]
    assert cv["late"].tolist() == [int(ev.sum() - cv["new_evacuated"].sum()), 0, E, 3 * E]
    for k in ("new_evacuated", "running", "ended", "alive"):
        assert np.array_equal(cv[k], sum(r[k] for r in cv["per_layout"])), k
    assert cv["new_evacuated"].sum() + cv["late"][0] == ev.sum()
    empty = build_curves({k: np.zeros((1, 3), np.int64) for k in tu.SLOTS}, np.zeros((1, 4)), 0, Pn)
    assert empty["episodes"] == 0 and np.isnan(empty["avg_health"]).all() and np.isnan(empty["evacuated_mean"]).all()


# ------------------------------------------------------------------ the C entries, no device
def _host_descriptor(E=4, T=8, n_rows=1, n_trk=0, leave_out=None):
    """An evx_timeline whose pointers are host scratch: only ever passed to calls that must fail
    before they launch anything."""
    from evacx._lib import evx_timeline
    keep = []
    d = evx_timeline(E=E, T=T, n_rows=n_rows, n_trk=n_trk)
    for name, _ in evx_timeline._fields_[4:]:
        if name == leave_out or (name.startswith("trk_") and not n_trk):
            continue
        buf = (ctypes.c_int64 * 64)()
        keep.append(buf)
        setattr(d, name, ctypes.addressof(buf))
    return d, keep


def test_library_exports_the_timeline_entries_and_the_descriptor_mirrors_the_header(tmp_path):
    import shutil
    import subprocess
    from golden_util import ROOT
    from evacx import _lib
    L = _lib.lib()
    for s in ("evx_timeline_init", "evx_timeline_update", "evx_timeline_trace0", "evx_timeline_last_error"):
        assert hasattr(L, s) and s in _lib.SIGNATURES, s
    S = _lib.evx_timeline
    assert ctypes.sizeof(S) == 16 + 17 * ctypes.sizeof(ctypes.c_void_p)
    cc = shutil.which("cc") or shutil.which("clang") or shutil.which("clang", path="/opt/rocm/llvm/bin")
    assert cc, "no C compiler (cc, clang) to check the structure layout with"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "evacx.h"', "int main(void) {",
             '    printf("%d\\n", (int)sizeof(evx_timeline));']
    lines += [f'    printf("%d\\n", (int)offsetof(evx_timeline, {f}));' for f, _ in S._fields_]
    src, exe = tmp_path / "tl.c", tmp_path / "tl"
    src.write_text("\n".join(lines + ["    return 0;", "}"]) + "\n")
    r = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]


def test_entries_refuse_before_any_launch():
    from evacx import _lib
    L = _lib.lib()
    err = L.evx_timeline_last_error
    cn, dn, pk, hl = ((ctypes.c_int64 * 64)() for _ in range(4))
    ref = ctypes.byref

    def upd(d, counts=cn, done=dn, pk_=pk, hl_=hl, P_=4):
        return L.evx_timeline_update(None if d is None else ref(d), counts, done, None, pk_, hl_, P_, 0, None)
    assert upd(None) == -22 and b"timeline_update: NULL timeline descriptor" in err()
    assert L.evx_timeline_init(None, None) == -22 and b"timeline_init: NULL timeline descriptor" in err()
    assert L.evx_timeline_trace0(None, pk, hl, 4, None) == -22 and b"timeline_trace0: NULL timeline descriptor" in err()
    assert err() == L.evx_last_error()  # the one thread-local error text
    for name in ("t", "n_total", "evac", "health_q", "late", "bad_health"):
        d, keep = _host_descriptor(leave_out=name)
        assert upd(d) == -22 and b"timeline_update: NULL timeline buffer" in err(), name
        assert L.evx_timeline_init(ref(d), None) == -22 and b"timeline_init: NULL timeline buffer" in err()
    d, keep = _host_descriptor()
    assert upd(d, counts=None) == -22 and b"NULL counts or done" in err()
    assert upd(d, done=None) == -22 and b"NULL counts or done" in err()
    for E, T in ((0, 8), (-1, 8), (4, 0), (4, -3)):
        d.E, d.T = E, T
        assert upd(d) == -22 and b"E and T must be >= 1" in err(), (E, T)
    d.E, d.T = 4, 8
    for Pn in (0, -1, 16384, 1 << 20):
        assert upd(d, P_=Pn) == -22 and b"P must be 1..16383" in err(), Pn
        assert L.evx_timeline_trace0(ref(d), pk, hl, Pn, None) == -22 and b"P must be 1..16383" in err()
    for rows in (0, -2):
        d.n_rows = rows
        assert upd(d) == -22 and b"n_rows must be >= 1" in err()
    d.n_rows = 1
    assert upd(d, pk_=None) == -22 and b"pk and health go together" in err()
    assert upd(d, hl_=None) == -22 and b"pk and health go together" in err()
    assert L.evx_timeline_trace0(ref(d), None, hl, 4, None) == -22 and b"NULL pk or health" in err()
    d.n_trk = 3  # tracked persons, no trace arrays
    assert upd(d) == -22 and b"tracked persons without their trace arrays" in err()
    assert L.evx_timeline_init(ref(d), None) == -22 and b"trace arrays" in err()
    for name in ("trk_env", "trk_person", "trk_pk", "trk_health", "trk_len"):
        d, keep = _host_descriptor(n_trk=3, leave_out=name)
        assert upd(d) == -22 and b"tracked persons without their trace arrays" in err(), name
    d, keep = _host_descriptor(n_trk=3)
    assert upd(d, pk_=None, hl_=None) == -22 and b"tracked persons need pk and health" in err()
    d.n_trk = -1
    assert upd(d) == -22 and b"n_trk" in err()


def test_front_ends_check_their_arguments_before_the_device():
    import torch
    from evacx.evaluate import evaluate
    from evacx.timeline import Timeline
    for bad in (dict(E=0, P=150), dict(E=8, P=0), dict(E=8, P=16384), dict(E=8, P=150, T=0), dict(E=8, P=150, cap=-1),
                dict(E=8, P=150, n_layouts=0), dict(E=8, P=150, n_layouts=2),
                dict(E=8, P=150, n_layouts=2, layout_idx=torch.zeros(7, dtype=torch.int32)),
                dict(E=1 << 23, P=16383), dict(E=1 << 16, P=1 << 10, cap=1 << 10),  # E * cap * P >= 2^36
                dict(E=8, P=150, track=151), dict(E=8, P=150, track=-1), dict(E=8, P=150, track=True),
                dict(E=8, P=150, track=([0, 8], [1, 2])), dict(E=8, P=150, track=([0, 1], [1, 150])),
                dict(E=8, P=150, track=([0], [1, 2]))):
        with pytest.raises(ValueError):
            Timeline(bad.pop("E"), "cuda", bad.pop("P"), **bad)
    with pytest.raises(ValueError, match="track needs timeline"):
        evaluate(None, 8, 1, 4, track=5)
    with pytest.raises(ValueError, match="track needs timeline"):
        evaluate(None, 8, 1, 4, metrics=True, track=([0], [0]))


def test_runner_takes_the_three_flags():
    from Louvre_Evacuation.runners import evaluate_vec
    a = evaluate_vec.parse_args([])
    assert (a.curves, a.track, a.plot) == (False, 0, False)
    a = evaluate_vec.parse_args(["--curves", "--track", "20", "--plot"])
    assert (a.curves, a.track, a.plot) == (True, 20, True)
    assert evaluate_vec.CURVE_COLUMNS[:2] == ["step", "time_s"] and "avg_health" in evaluate_vec.CURVE_COLUMNS


def test_write_curves_round_trips(tmp_path):
    import csv
    from Louvre_Evacuation.runners import evaluate_vec
    tr, pk, eps = tu.fixture("cfg1_single_traj")
    a, b = eps[1]
    _, cv = _episode_curves("cfg1_single_traj", a, b)
    n = evaluate_vec.write_curves(tmp_path / "c.csv", cv)
    rows = list(csv.reader(open(tmp_path / "c.csv")))
    assert n == b - a and rows[0] == evaluate_vec.CURVE_COLUMNS and len(rows) == n + 1
    for s, row in enumerate(rows[1:]):
        for k, v in zip(evaluate_vec.CURVE_COLUMNS, row):
            assert float(v) == cv[k][s], (s, k)


def test_runner_writes_its_files_and_goes_on_without_matplotlib(tmp_path, capsys, monkeypatch):
    import argparse
    import sys
    from evacx.layout import reference_single
    from Louvre_Evacuation.runners import evaluate_vec
    a, b = tu.fixture("cfg1_single_traj")[2][0]
    _, cv = _episode_curves("cfg1_single_traj", a, b)
    ev = {"curves": cv, "episodes": 1}
    args = argparse.Namespace(curves=True, track=150, plot=True)
    monkeypatch.setitem(sys.modules, "matplotlib", None)  # importing it now raises ImportError
    evaluate_vec.write_outputs(args, str(tmp_path), "static", ev, reference_single())
    text = capsys.readouterr().out
    assert "--plot needs matplotlib" in text and not list(tmp_path.glob("*.png"))
    assert (tmp_path / "curves_static.csv").stat().st_size > 0
    z = np.load(tmp_path / "tracked_static.npz")
    assert np.array_equal(z["x"], cv["tracked"]["x"]) and z["len"].tolist() == [b - a + 1] * P


def test_runner_writes_the_figure(tmp_path):
    pytest.importorskip("matplotlib")
    import argparse
    from evacx.layout import reference_single
    from Louvre_Evacuation.runners import evaluate_vec
    a, b = tu.fixture("cfg1_multi_traj")[2][0]
    _, cv = _episode_curves("cfg1_multi_traj", a, b)
    args = argparse.Namespace(curves=False, track=0, plot=True)
    evaluate_vec.write_outputs(args, str(tmp_path), "static", {"curves": cv, "episodes": 1}, reference_single())
    assert (tmp_path / "evaluation_static.png").read_bytes()[:4] == b"\x89PNG"
    assert not (tmp_path / "curves_static.csv").exists()


def test_plot_evaluation_writes_a_png(tmp_path):
    pytest.importorskip("matplotlib")
    from evacx.layout import reference_single
    from Louvre_Evacuation.utils.visualization import plot_evaluation
    a, b = tu.fixture("cfg1_single_traj")[2][0]
    _, cv = _episode_curves("cfg1_single_traj", a, b)
    for i, (result, kw) in enumerate((({"curves": cv, "episodes": 1}, dict(layout=reference_single(), title="static")),
                                      ({k: v for k, v in cv.items() if k != "tracked"}, {}))):
        path = tmp_path / f"fig{i}.png"
        plot_evaluation(result, str(path), **kw)
        data = path.read_bytes()
        assert len(data) > 10000 and data[:8] == b"\x89PNG\r\n\x1a\n"
