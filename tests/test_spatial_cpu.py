"""The spatial maps without a GPU: the numpy restatement (spatial_util.spatial_ref) on a hand-built
case and against the reference's own heat map in the trajectory fixtures, maps()'s post-processing
on made-up counts, and the plan and the refusals of the C ABI (no launch, no device)."""
import ctypes

import numpy as np
import pytest

import spatial_util as su
from golden_util import load


def _word(x, y, flags=0):
    return x | (y << 12) | (flags << 24)


def _cells(a):
    """{(row, x, y): count} of the non-zero cells."""
    return {tuple(int(v) for v in i): int(a[tuple(i)]) for i in np.argwhere(a)}


# ------------------------------------------------------------------ the restatement, by hand
def test_hand_built_case_covers_every_class_cap_bad_and_the_row_clamp():
    """Two envs of three persons and one robot on a 4 x 3 grid, four steps, cap = 1. Env 0 (row 0)
    finishes at step 2 and is not counted afterwards; env 1 has layout_idx 7, clamped to row 1."""
    S, D = 1, 2
    ref = su.spatial_ref(2, 3, 1, 4, 3, n_rows=2, layout_idx=[0, 7], cap=1)
    ref.sync(np.array([[_word(0, 0), _word(1, 1), _word(2, 2)],
                       [_word(1, 0), _word(1, 0), _word(0, 2)]], np.uint32))
    # step 1. env 0: arrive (0,1), stall (1,1), evac (3,2). env 1: three stalls, two on one cell.
    ref.update(np.array([[_word(0, 1), _word(1, 1), _word(3, 2, S)],
                         [_word(1, 0), _word(1, 0), _word(0, 2)]], np.uint32),
               su.pack_robots([[[1, 0]], [[0, 0]]]), [0, 0])
    # step 2. env 0: died (0,1) without moving, a live person outside the grid, a safe one left
    # alone, the robot outside the grid, done. env 1: two arrivals on one cell; safe and dead at
    # once counts as evac, and it did not move.
    ref.update(np.array([[_word(0, 1, D), _word(5, 1), _word(3, 2, S)],
                         [_word(1, 1), _word(1, 1), _word(0, 2, S | D)]], np.uint32),
               su.pack_robots([[[9, 0]], [[0, 0]]]), [1, 0])
    assert ref.n_total.tolist() == [1, 0]
    after_reset = np.array([[_word(2, 0), _word(2, 1), _word(2, 2)],
                            [_word(3, 2), _word(3, 2), _word(3, 2)]], np.uint32)  # env 1's row: masked out
    ref.sync(after_reset, mask=[1, 0])
    assert ref.prev[1].tolist() == [_word(1, 1), _word(1, 1), _word(0, 2, S | D)]
    # step 3. env 0 is past its cap: nothing of it is counted, prev still follows.
    ref.update(np.array([[_word(3, 0), _word(2, 1), _word(2, 2)],
                         [_word(1, 1), _word(2, 1), _word(0, 2, S | D)]], np.uint32),
               su.pack_robots([[[2, 2]], [[0, 1]]]), [0, 0])
    # step 4. env 1: moved and died (1,2), stall (2,1), done.
    last = np.array([[_word(3, 0), _word(2, 1), _word(2, 2)],
                     [_word(1, 2, D), _word(2, 1), _word(0, 2, S | D)]], np.uint32)
    ref.update(last, su.pack_robots([[[2, 2]], [[0, 1]]]), [0, 1])
    assert _cells(ref.arrive) == {(0, 0, 1): 1, (1, 1, 1): 2, (1, 2, 1): 1}
    assert _cells(ref.stall) == {(0, 1, 1): 1, (1, 1, 0): 2, (1, 0, 2): 1, (1, 1, 1): 1, (1, 2, 1): 1}
    assert _cells(ref.evac) == {(0, 3, 2): 1, (1, 0, 2): 1}
    assert _cells(ref.died) == {(0, 0, 1): 1, (1, 1, 2): 1}
    assert _cells(ref.robot) == {(0, 1, 0): 1, (1, 0, 0): 2, (1, 0, 1): 2}
    assert ref.steps.tolist() == [2, 4] and ref.bad.tolist() == [2] and ref.n_total.tolist() == [1, 1]
    assert ref.episodes().tolist() == [1, 1] and np.array_equal(ref.prev, last)
    # without the cap env 0's second episode counts too: one more arrival, two stalls per step
    free = su.spatial_ref(1, 3, 1, 4, 3)
    free.n_total[0] = 1
    free.sync(after_reset[:1])
    free.update(last[:1], su.pack_robots([[[2, 2]]]), [0])
    assert _cells(free.arrive) == {(0, 3, 0): 1} and _cells(free.stall) == {(0, 2, 1): 1, (0, 2, 2): 1}


# ------------------------------------------------------------------ against the reference's heat map
# what the issue's throwaway script found; the test derives each figure again from the fixture
FIXTURE_TOTALS = {"cfg1_single_traj": dict(flow=3860, stall=6957, evac=168, died=282),
                  "cfg1_multi_traj": dict(flow=3149, stall=5656, evac=151, died=149)}


@pytest.mark.parametrize("name", sorted(FIXTURE_TOTALS))
def test_restatement_agrees_with_the_reference_heat_map(name):
    """People.thmap takes 1 at the new cell of every person that moved (envs/people.py:309) and 1 at
    the cell of every person that lost a conflict over a target and stayed (people.py:248-249). So
    per step and cell: 0 <= d thmap - (arrive + evac) <= stall, while every newly safe person moved
    and nobody moves in the step it dies; both are asserted of the fixture."""
    tr = load(name)
    pk = su.fixture_pk(tr)
    n, P = pk.shape
    GX, GY = tr["snap_thmap"].shape[1:]
    R = tr["snap_robots"].shape[1]
    ref = su.spatial_ref(1, P, R, GX, GY)
    tot = dict(flow=0, stall=0, evac=0, died=0)
    steps = 0
    for k in range(n):
        if tr["is_reset"][k]:
            ref.sync(pk[k][None])
            continue
        before = {m: getattr(ref, m)[0].copy() for m in su.MAPS}
        ox, oy, osafe, odead = su.decode(pk[k - 1])
        x, y, safe, dead = su.decode(pk[k])
        moved = (x != ox) | (y != oy)
        assert not (osafe & ~safe).any() and not (odead & ~dead).any()  # absorbing
        assert moved[safe & ~osafe].all(), "a newly safe person that did not move"
        assert not moved[dead & ~odead & ~safe].any(), "a person that moved in the step it died"
        assert not moved[osafe | odead].any()
        ref.update(pk[k][None], su.pack_robots(tr["snap_robots"][k])[None], [tr["done"][k]])
        d = {m: getattr(ref, m)[0] - before[m] for m in su.MAPS}
        flow = d["arrive"] + d["evac"]
        extra = tr["snap_thmap"][k].astype(np.int64) - tr["snap_thmap"][k - 1] - flow
        assert (extra >= 0).all() and (extra <= d["stall"]).all(), k
        assert d["robot"].sum() == R
        for m in tot:
            tot[m] += int((flow if m == "flow" else d[m]).sum())
        steps += 1
    assert ref.bad[0] == 0 and ref.steps[0] == steps and ref.robot.sum() == steps * R
    assert ref.n_total[0] == tr["done"].sum() == tr["is_reset"].sum()
    ends = np.nonzero(tr["done"])[0]
    assert ref.evac.sum() == tr["evac"][ends].sum() and ref.died.sum() == tr["dead"][ends].sum()
    assert tot == FIXTURE_TOTALS[name]
    # occupancy is the live persons after every step
    live_after = sum(int((tr["snap_flags"][k] == 0).sum()) for k in range(n) if not tr["is_reset"][k])
    assert (ref.arrive + ref.stall).sum() == live_after


def test_synthetic_sequence_exercises_every_class_and_bad():
    """The sequence the GPU tests feed has every class, persons and a robot outside the grid."""
    first, seq = su.synthetic(65)
    E, P = first.shape
    ref = su.spatial_ref(E, P, 2, 12, 9, n_rows=3, layout_idx=np.arange(E) % 3, cap=2)
    ref.sync(first)
    for pk, robots, done, nxt in seq:
        ref.update(pk, robots, done)
        ref.sync(nxt, mask=done)
    assert all(getattr(ref, m).sum() > 0 for m in su.MAPS) and ref.bad[0] >= 3
    assert (ref.n_total > 2).any() and ref.steps.sum() < E * len(seq)  # the cap kept later episodes out
    assert all((getattr(ref, m).sum(axis=(1, 2)) > 0).all() for m in ("arrive", "stall", "robot"))


# ------------------------------------------------------------------ maps() post-processing
def test_build_maps_orders_exits_breaks_hotspot_ties_and_marks_empty_cells():
    from evacx.spatial import build_maps
    GX, GY = 5, 4
    c = {m: np.zeros((2, GX, GY), np.int64) for m in su.MAPS}
    c["evac"][0, 4, 1], c["evac"][0, 4, 2], c["evac"][0, 0, 3], c["evac"][1, 4, 2] = 6, 10, 6, 4
    c["stall"][0, 1, 1], c["stall"][0, 3, 0], c["stall"][0, 2, 2] = 7, 7, 9
    c["arrive"][0, 1, 1], c["arrive"][0, 0, 0] = 7, 3
    c["stall"][1] = np.arange(GX * GY).reshape(GX, GY) // 2  # pairs of equal counts: ties
    out = build_maps(c, steps=[4, 0], episodes=[2, 0], bad=5)
    assert set(out) == {0, 1, "sum", "bad"} and out["bad"] == 5
    r0 = out[0]
    assert r0["exit_use"] == [(4, 2, 10, 10 / 22), (0, 3, 6, 6 / 22), (4, 1, 6, 6 / 22)]
    assert r0["hotspots"] == [(2, 2, 9), (1, 1, 7), (3, 0, 7)]  # the tie by cell index, and only stall > 0
    assert np.array_equal(r0["occupancy"], c["arrive"][0] + c["stall"][0])
    assert r0["density"][1, 1] == 14 / 4 and r0["steps"] == 4 and r0["episodes"] == 2
    ratio = r0["stall_ratio"]
    assert ratio[1, 1] == 0.5 and ratio[0, 0] == 0.0 and ratio[2, 2] == 1.0
    assert np.isnan(ratio).sum() == GX * GY - 4 and np.isnan(ratio[4, 3])
    r1 = out[1]
    assert np.isnan(r1["density"]).all() and r1["exit_use"] == [(4, 2, 4, 1.0)]
    assert len(r1["hotspots"]) == 10 and r1["hotspots"][:4] == [(4, 2, 9), (4, 3, 9), (4, 0, 8), (4, 1, 8)]
    s = out["sum"]
    assert s["steps"] == 4 and s["episodes"] == 2
    for m in su.MAPS:
        assert np.array_equal(s[m], c[m].sum(axis=0))
    assert s["exit_use"][0] == (4, 2, 14, 14 / 26) and out[0]["evac"].dtype == np.int64
    empty = build_maps({m: np.zeros((1, 2, 2), np.int64) for m in su.MAPS}, [0], [0], 0)
    assert empty["sum"]["exit_use"] == [] and empty["sum"]["hotspots"] == []


# ------------------------------------------------------------------ the C ABI without a device
def test_plan_changes_route_where_the_two_maps_leave_the_lds():
    from evacx import spatial
    lds = spatial.plan(89, 230, 150)  # G = 20470: 64 + 8 G = 163 824 bytes, 16 short of 160 KiB
    assert lds["route"] == "LDS" and lds["bands"] == 1 and lds["launches"] == 1 and lds["band_w"] == 89
    assert lds["band_cells"] == 89 * 230 and lds["lds_bytes"] == 64 + 8 * 89 * 230 <= 160 * 1024
    bands = spatial.plan(89, 231, 150)  # G = 20559: 8 bytes per cell no longer fit
    assert bands["route"] == "BANDS" and bands["bands"] == 2 and bands["launches"] == 2 and bands["band_w"] == 45
    cfg3 = spatial.plan(130, 130, 2276)
    assert cfg3["route"] == "LDS" and cfg3["lds_bytes"] == 64 + 8 * 16900 and cfg3["envs_per_wg"] == 128
    cfg4 = spatial.plan(258, 258, 50)
    assert cfg4["route"] == "BANDS" and cfg4["bands"] == 4 and cfg4["band_w"] == 65
    for pl in (lds, bands, cfg3, cfg4, spatial.plan(4096, 4096, 1), spatial.plan(1, 1, 16383)):
        assert pl["band_cells"] == pl["band_w"] * (pl["band_cells"] // pl["band_w"])
        assert pl["lds_bytes"] == 64 + 8 * pl["band_cells"] <= 160 * 1024 and pl["threads"] == 1024
        # a u32 counter holds a whole share, whatever pk holds
        assert 16 <= pl["envs_per_wg"] <= 1024 and pl["envs_per_wg"] * 16383 < 2 ** 32
    assert spatial.plan(4096, 4096, 1)["bands"] * spatial.plan(4096, 4096, 1)["band_w"] >= 4096


def _descriptor(**kw):
    from evacx import _lib
    one = 8  # any non-NULL address: a refused call reads no array
    d = dict(E=4, P=10, R=2, GX=12, GY=9, n_rows=1, prev=one, n_total=one, arrive=one, stall=one, evac=one,
             died=one, robot=one, steps=one, bad=one)
    d.update(kw)
    return _lib.evx_spatial(**d)


REFUSED = {
    "E < 1": (dict(E=0), b"E must be >= 1"),
    "P = 0": (dict(P=0), b"P must be 1..16383"),
    "P too large": (dict(P=16384), b"P must be 1..16383"),
    "GX too large": (dict(GX=4097), b"GX and GY must be 1..4096"),
    "GY too large": (dict(GY=4097), b"GX and GY must be 1..4096"),
    "n_rows < 1": (dict(n_rows=0), b"n_rows must be >= 1"),
    "R < 0": (dict(R=-1), b"R must be >= 0"),
    "NULL map": (dict(stall=None), b"NULL spatial buffer"),
    "NULL prev": (dict(prev=None), b"NULL spatial buffer"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_bad_descriptors_are_refused_before_any_launch(case):
    from evacx import _lib
    L = _lib.lib()
    kw, text = REFUSED[case]
    d = _descriptor(**kw)
    for call in (lambda: L.evx_spatial_init(ctypes.byref(d), None),
                 lambda: L.evx_spatial_sync(ctypes.byref(d), 8, None, None),
                 lambda: L.evx_spatial_update(ctypes.byref(d), 8, 8, 8, None, 0, None)):
        assert call() == -22
        assert text in L.evx_spatial_last_error() and L.evx_spatial_last_error() == L.evx_last_error()


def test_bad_arguments_are_refused_before_any_launch():
    from evacx import _lib
    L = _lib.lib()
    d = _descriptor()
    cases = [(lambda: L.evx_spatial_init(None, None), b"spatial_init: NULL spatial descriptor"),
             (lambda: L.evx_spatial_update(None, 8, 8, 8, None, 0, None), b"spatial_update: NULL spatial descriptor"),
             (lambda: L.evx_spatial_sync(ctypes.byref(d), None, None, None), b"spatial_sync: NULL pk"),
             (lambda: L.evx_spatial_update(ctypes.byref(d), None, 8, 8, None, 0, None), b"NULL pk or done"),
             (lambda: L.evx_spatial_update(ctypes.byref(d), 8, 8, None, None, 0, None), b"NULL pk or done"),
             (lambda: L.evx_spatial_update(ctypes.byref(d), 8, None, 8, None, 0, None), b"NULL robots with R > 0"),
             (lambda: L.evx_spatial_plan(12, 9, 10, 1, None), b"spatial_plan: NULL plan"),
             (lambda: L.evx_spatial_plan(12, 4097, 10, 1, ctypes.byref(_lib.evx_spatial_launch())), b"1..4096"),
             (lambda: L.evx_spatial_plan(12, 9, 0, 1, ctypes.byref(_lib.evx_spatial_launch())), b"P must be")]
    for call, text in cases:
        assert call() == -22
        assert text in L.evx_spatial_last_error(), (text, L.evx_spatial_last_error())


def test_spatial_maps_refuses_bad_sizes_in_python():
    from evacx.spatial import Grid, SpatialMaps
    for grid, kw in ((Grid(12, 9, 0, 1), {}), (Grid(4097, 9, 5, 1), {}), (Grid(12, 9, 5, -1), {}),
                     (Grid(12, 9, 5, 1), dict(cap=-1)), (Grid(12, 9, 5, 1), dict(n_layouts=2)),
                     (Grid(12, 9, 5, 1), dict(n_layouts=0))):
        with pytest.raises(ValueError, match="SpatialMaps"):
            SpatialMaps(4, "cpu", grid, **kw)


# ------------------------------------------------------------------ the runner's files, from fixture maps
def _fixture_maps(name="cfg1_multi_traj"):
    from evacx.spatial import build_maps
    tr = load(name)
    pk = su.fixture_pk(tr)
    GX, GY = tr["snap_thmap"].shape[1:]
    ref = su.spatial_ref(1, pk.shape[1], tr["snap_robots"].shape[1], GX, GY)
    for k in range(len(pk)):
        if tr["is_reset"][k]:
            ref.sync(pk[k][None])
        else:
            ref.update(pk[k][None], su.pack_robots(tr["snap_robots"][k])[None], [tr["done"][k]])
    return build_maps({m: getattr(ref, m) for m in su.MAPS}, ref.steps, ref.episodes(), int(ref.bad[0])), ref


def test_runner_writes_the_maps_and_goes_on_without_matplotlib(tmp_path, capsys, monkeypatch):
    import argparse
    import sys
    from evacx.layout import reference_multi
    from Louvre_Evacuation.runners import evaluate_vec
    maps, ref = _fixture_maps()
    monkeypatch.setitem(sys.modules, "matplotlib", None)  # importing it now raises ImportError
    evaluate_vec.write_maps(argparse.Namespace(plot=True), str(tmp_path), "static", {"maps": maps, "episodes": 3},
                            reference_multi())
    text = capsys.readouterr().out
    assert "--plot needs matplotlib" in text and not list(tmp_path.glob("*.png"))
    z = np.load(tmp_path / "maps_static.npz")
    assert sorted(z.files) == sorted(evaluate_vec.MAPS_KEYS)
    for m in su.MAPS:
        assert np.array_equal(z[m], getattr(ref, m)[0]), m
    assert z["steps"] == ref.steps[0] and z["episodes"] == ref.n_total[0] == 2 and z["bad"] == 0
    # the fixture's 151 evacuated left through the cells around the reference layout's exit (36, 15)
    use = z["exit_use"]
    assert use[:, 2].sum() == 151 and abs(use[:, 3].sum() - 1) < 1e-12 and (np.diff(use[:, 2]) <= 0).all()
    assert (np.abs(use[:, 0] - 36) <= 1).all() and (np.abs(use[:, 1] - 15) <= 1).all()
    first = f"static: exit use ({int(use[0, 0])},{int(use[0, 1])}) {use[0, 2] / 151:.1%}, "
    assert first in text and "; top stall cell (" in text
    x, y, n = z["hotspots"][0]
    assert n == ref.stall.max() == ref.stall[0, x, y] and f"({x},{y}) with {n} person-steps" in text


def test_plot_maps_writes_a_png(tmp_path):
    pytest.importorskip("matplotlib")
    from evacx.layout import reference_multi
    from Louvre_Evacuation.utils.visualization import plot_maps
    maps, _ = _fixture_maps()
    for i, (result, kw) in enumerate((({"maps": maps}, dict(layout=reference_multi(), title="static")),
                                      (maps, dict(row=0)))):
        path = tmp_path / f"maps{i}.png"
        plot_maps(result, str(path), **kw)
        data = path.read_bytes()
        assert len(data) > 10000 and data[:8] == b"\x89PNG\r\n\x1a\n"
