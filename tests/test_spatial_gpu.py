"""Spatial maps on the device (csrc/spatial.hip, evacx.spatial), evaluate(maps=True) and the runner's
--maps.

The reference everywhere is spatial_util.spatial_ref, the update restated in numpy and fed from the
host -- the fixtures' own records, made-up pk sequences, or the state read back from a second
VecEnv -- never SpatialMaps itself. Every number is an integer count and is compared exactly."""
import numpy as np
import pytest
import torch

import spatial_util as su

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
PAD = 512  # sentinel bytes behind every array


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_arrays(sm):
    torch.cuda.synchronize()
    out = {k: getattr(sm, k).cpu().numpy() for k in ("prev", "n_total", *su.MAPS, "steps", "bad")}
    out["prev"] = out["prev"].view(np.uint32)
    return out


def _assert_equals_ref(sm, ref):
    got, want = _device_arrays(sm), ref.arrays()
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), \
            (k, np.argwhere(got[k] != want[k])[:8], got[k].sum(), want[k].sum())
    return got


def _padded(sm):
    """Every array of the maps moved in front of sentinel bytes and initialised again; the backing buffers."""
    import ctypes
    from evacx import _lib
    backing = {}
    for k in ("prev", "n_total", *su.MAPS, "steps", "bad"):
        old = getattr(sm, k)
        nbytes = old.numel() * old.element_size()
        buf = torch.full((nbytes + PAD,), SENTINEL, dtype=torch.uint8, device=old.device)
        new = buf[:nbytes].view(old.dtype).view(old.shape)
        setattr(sm, k, new)
        setattr(sm.c, k, new.data_ptr())
        backing[k] = (buf, nbytes)
    _lib.check(_lib.lib().evx_spatial_init(ctypes.byref(sm.c), None), "spatial_init")
    return backing


# ------------------------------------------------------------------ 1: the reference trajectories
@pytest.mark.parametrize("name", ["cfg1_single_traj", "cfg1_multi_traj"])
def test_replayed_fixture_records_give_the_restated_maps(name):
    """E = 5 copies of the fixture's records, started at different offsets (the record index wraps),
    so the envs are at different episode phases; a record with is_reset is synced, not counted."""
    _need_gpu()
    from golden_util import load
    from evacx.spatial import Grid, SpatialMaps
    tr = load(name)
    pk = su.fixture_pk(tr)
    n, P = pk.shape
    GX, GY = tr["snap_thmap"].shape[1:]
    R = tr["snap_robots"].shape[1]
    E, offsets = 5, np.array([0, 7, 31, 64, 100])
    sm = SpatialMaps(E, "cuda", Grid(GX, GY, P, R))
    ref = su.spatial_ref(E, P, R, GX, GY)
    rob = su.pack_robots(tr["snap_robots"])
    for s in range(n):
        k = (offsets + s) % n
        reset = tr["is_reset"][k]
        step = ~reset
        state = (_dev(pk[k].view(np.int32)).view(-1), _dev(rob[k]).view(-1))
        if s == 0:  # every env starts from its record, whatever it is
            sm.sync(state)
            ref.sync(pk[k])
            continue
        # one call counts every env, so an env on a reset record gets its previous record again
        # (nothing moves, no env-step is lost from the comparison: the restatement gets the same)
        word = np.where(reset[:, None], ref.prev, pk[k])
        done = (tr["done"][k] & step).astype(np.uint8)
        state = (_dev(word.view(np.int32)).view(-1), state[1])
        sm.update(state, _dev(done))
        ref.update(word, rob[k], done)
        if reset.any():
            mask = reset.astype(np.uint8)
            sm.sync((_dev(pk[k].view(np.int32)).view(-1), None), _dev(mask))
            ref.sync(pk[k], mask)
    got = _assert_equals_ref(sm, ref)
    assert got["bad"][0] == 0 and got["evac"].sum() > 100 and got["died"].sum() > 100
    assert got["steps"][0] == E * (n - 1) and sm.plan()["route"] == "LDS"


# ------------------------------------------------------------------ 2: made-up pk, no env
def _run_synthetic(P, GX=12, GY=9, E=37, steps=12, padded=True):
    from evacx.spatial import Grid, SpatialMaps
    R, cap = 2, 2
    lidx = (np.arange(E) % 3).astype(np.int32)
    lidx[E - 1] = 9  # out of range: clamped to row 2
    sm = SpatialMaps(E, "cuda", Grid(GX, GY, P, R), layout_idx=_dev(lidx), n_layouts=3, cap=cap)
    backing = _padded(sm) if padded else {}
    ref = su.spatial_ref(E, P, R, GX, GY, n_rows=3, layout_idx=lidx, cap=cap)
    first, seq = su.synthetic(P, E=E, R=R, GX=GX, GY=GY, steps=steps)
    sm.sync((_dev(first).view(-1), None))
    ref.sync(first)
    for word, robots, done, nxt in seq:
        sm.update((_dev(word).view(-1), _dev(robots).view(-1)), _dev(done))
        ref.update(word, robots, done)
        sm.sync((_dev(nxt).view(-1), None), _dev(done))
        ref.sync(nxt, done)
    torch.cuda.synchronize()
    for k, (buf, nbytes) in backing.items():
        assert (buf[nbytes:] == SENTINEL).all().item(), f"{k}: written past its end"
    return sm, ref


@pytest.mark.parametrize("P", [1, 63, 64, 65, 569])
def test_synthetic_steps_equal_the_numpy_restatement_and_repeat(P):
    _need_gpu()
    sm, ref = _run_synthetic(P)
    got = _assert_equals_ref(sm, ref)
    assert got["bad"][0] >= 3 and got["robot"].sum() <= got["steps"].sum() * 2
    assert (got["n_total"] > 2).any() and got["steps"].sum() < 37 * 12  # the cap kept later episodes out
    assert (got["steps"] > 0).all() and sm.plan()["route"] == "LDS"
    assert np.array_equal(sm.episodes(), ref.episodes())
    again = _device_arrays(_run_synthetic(P)[0])
    for k in got:
        assert np.array_equal(again[k], got[k]), k


# ------------------------------------------------------------------ 3: contention
def test_every_person_on_one_cell_adds_up_exactly():
    """E * P = 145 664 adds per step onto one counter: a workgroup's share alone is 16 * 2276 adds."""
    _need_gpu()
    from evacx.spatial import Grid, SpatialMaps
    E, P, GX, GY = 64, 2276, 12, 9
    rng = np.random.default_rng(3)
    start = (rng.integers(0, 5, (E, P)) | (rng.integers(0, GY, (E, P)) << 12)).astype(np.int32)
    there = np.full((E, P), 7 | (4 << 12), np.int32)
    sm = SpatialMaps(E, "cuda", Grid(GX, GY, P, 0))
    assert sm.plan()["envs_per_wg"] == 16
    sm.sync((_dev(start).view(-1), None))
    done = torch.zeros(E, dtype=torch.uint8, device="cuda")
    for s in range(3):
        sm.update((_dev(there).view(-1), None), done)
        got = _device_arrays(sm)
        want = np.zeros((1, GX, GY), np.int64)
        want[0, 7, 4] = E * P
        assert np.array_equal(got["arrive"], want), s
        assert np.array_equal(got["stall"], want * s), s
    assert got["steps"][0] == 3 * E and got["bad"][0] == 0 and not got["evac"].any() and not got["robot"].any()
    assert np.array_equal(got["prev"], there.view(np.uint32))


# ------------------------------------------------------------------ 4: both routes
@pytest.mark.parametrize("grid,route,bands", [((89, 230), "LDS", 1), ((89, 231), "BANDS", 2)])
def test_the_route_changes_where_the_plan_says_and_both_sides_are_exact(grid, route, bands):
    _need_gpu()
    GX, GY = grid
    sm, ref = _run_synthetic(65, GX=GX, GY=GY, E=37, steps=6)
    pl = sm.plan()
    assert (pl["route"], pl["bands"], pl["launches"]) == (route, bands, 1 if bands == 1 else 2)
    got = _assert_equals_ref(sm, ref)
    assert got["arrive"].sum() > 0 and got["bad"][0] >= 2
    if bands > 1:  # persons on both sides of the cut were counted
        w = pl["band_w"]
        assert got["arrive"][:, :w].sum() > 0 and got["arrive"][:, w:].sum() > 0


def test_a_grid_beyond_the_lds_runs_in_bands():
    """258 x 258 (G = 66 564): four bands of 65, 65, 65 and 63 columns."""
    _need_gpu()
    sm, ref = _run_synthetic(50, GX=258, GY=258, E=4, steps=6)
    pl = sm.plan()
    assert pl["route"] == "BANDS" and pl["bands"] == 4 and pl["band_w"] == 65
    got = _assert_equals_ref(sm, ref)
    assert all(got["arrive"][:, 65 * b:65 * (b + 1)].sum() > 0 for b in range(4))


# ------------------------------------------------------------------ 5: evaluate(maps=True)
def _host_loop(lay, E, K, seed, steps, layout_of=None, n_rows=1):
    """A second VecEnv under the random policy's actions, its state read back every step."""
    from evacx import _lib
    from evacx.env import VecEnv, _stream
    env = VecEnv(lay, E, layout_of=layout_of)
    env.seed([1234 + i for i in range(E)])
    env.reset()
    ref = su.spatial_ref(E, lay.P, lay.R, lay.GX, lay.GY, n_rows=n_rows, layout_idx=layout_of, cap=K)
    ref.sync(env.pk.cpu().numpy())
    n = E * lay.R
    actions = torch.zeros(n, dtype=torch.int32, device="cuda")
    q0 = torch.zeros(n, 5, dtype=torch.float32, device="cuda")
    for s in range(steps):
        _lib.check(_lib.lib().evx_act(q0.data_ptr(), n, 5, 1.0, seed, s * n, actions.data_ptr(), _stream()), "act")
        env.step(actions, auto_reset=False)
        done = env.done.cpu().numpy()
        ref.update(env.pk.cpu().numpy(), env.robots.cpu().numpy(), done)
        env.reset(mask=env.done)
        ref.sync(env.pk.cpu().numpy(), done)
    env.check_err()
    return ref


def _assert_maps_equal_ref(maps, ref):
    for r in range(ref.n_rows):
        for m in su.MAPS:
            assert np.array_equal(maps[r][m], getattr(ref, m)[r]), (r, m)
        assert maps[r]["steps"] == ref.steps[r] and maps[r]["episodes"] == ref.episodes()[r]
    for m in su.MAPS:
        assert np.array_equal(maps["sum"][m], getattr(ref, m).sum(axis=0)), m
    assert maps["sum"]["steps"] == ref.steps.sum() and maps["bad"] == ref.bad[0] == 0


def _same_results(off, on, extra):
    assert set(on) - set(off) == extra
    for k in off:
        if k == "per_env":
            for name, x in off[k].items():
                y = on[k][name]
                assert torch.equal(x.view(torch.int64), y.view(torch.int64)) if x.dtype == torch.float64 \
                    else torch.equal(x, y), name
        else:
            assert off[k] == on[k], k


def test_evaluate_with_maps_leaves_the_trajectory_alone_and_matches_a_host_loop():
    _need_gpu()
    from golden_util import traj_tables
    from evacx.env import DeviceLayout
    from evacx.evaluate import evaluate
    tables, P = traj_tables("cfg1_single_traj")
    lay = DeviceLayout(tables, P)
    E, K = 6, 2
    off = evaluate(lay, E, K, "random")
    on = evaluate(lay, E, K, "random", maps=True)
    _same_results(off, on, {"maps"})
    maps = on["maps"]
    assert set(maps) == {0, "sum", "bad"}
    ref = _host_loop(lay, E, K, 0, on["steps"])
    _assert_maps_equal_ref(maps, ref)
    m = maps["sum"]
    assert m["evac"].sum() == int(on["per_env"]["w_evac"].sum()) == on["evacuated"]
    assert m["died"].sum() == int(on["per_env"]["w_dead"].sum()) == on["dead"]
    exit_bit = (lay.t["cellinfo"].cpu().numpy().reshape(lay.GX, lay.GY) & 2) != 0
    assert m["evac"].sum() > 0 and not m["evac"][~exit_bit].any()
    assert m["robot"].sum() == m["steps"] * lay.R and m["steps"] == int(on["per_env"]["w_len"].sum())
    assert m["episodes"] == E * K == on["episodes"]
    assert np.array_equal(m["occupancy"], m["arrive"] + m["stall"])
    assert sum(c for _, _, c, _ in m["exit_use"]) == on["evacuated"]
    # with the other device statistics as well: the same maps
    both = evaluate(lay, E, K, "random", metrics=True, timeline=True, maps=True)
    for k in su.MAPS:
        assert np.array_equal(both["maps"]["sum"][k], m[k]), k
    assert "curves" in both and both["avg_health"] is not None


def test_evaluate_with_maps_keeps_one_row_per_layout():
    _need_gpu()
    import dataclasses
    from evacx.env import DeviceLayout, LayoutSet
    from evacx.evaluate import evaluate
    from evacx.layout import build_tables, reference_multi
    spec = reference_multi()
    other = dataclasses.replace(spec, exit=(36, 5))
    lays = LayoutSet([DeviceLayout(build_tables(spec), 60), DeviceLayout(build_tables(other), 60)])
    E, K = 6, 2
    layout_of = [0, 1, 0, 1, 1, 0]
    off = evaluate(lays, E, K, "random", layout_of=layout_of)
    on = evaluate(lays, E, K, "random", layout_of=layout_of, maps=True)
    _same_results(off, on, {"maps"})
    maps = on["maps"]
    assert set(maps) == {0, 1, "sum", "bad"}
    ref = _host_loop(lays, E, K, 0, on["steps"], layout_of=layout_of, n_rows=2)
    _assert_maps_equal_ref(maps, ref)
    for r in (0, 1):
        assert maps[r]["evac"].sum() == on["per_layout"][r]["evacuated"] > 0
        assert maps[r]["episodes"] == 3 * K
        exit_bit = (lays.layouts[r].t["cellinfo"].cpu().numpy().reshape(lays.GX, lays.GY) & 2) != 0
        assert not maps[r]["evac"][~exit_bit].any()  # each row's people left through its own layout's exit
    assert not (maps[0]["evac"] > 0)[maps[1]["evac"] > 0].any()


# ------------------------------------------------------------------ 6: the runner
def _small_config(tmp_path):
    cfg = tmp_path / "small.yaml"
    cfg.write_text("env:\n  width: 36\n  height: 30\n  fire_zones: [[18, 14]]\n  exit_location: [36, 15]\n"
                   "  num_people: 40\nagent:\n  gamma: 0.99\nsave_path: \"unused\"\n")
    return cfg


def test_evaluate_vec_writes_the_maps_and_prints_its_line(tmp_path, capsys):
    _need_gpu()
    pytest.importorskip("matplotlib")
    from evacx.env import DeviceLayout
    from evacx.evaluate import evaluate
    from evacx.layout import build_tables
    from Louvre_Evacuation.runners import evaluate_vec
    out = tmp_path / "out"
    evaluate_vec.main(["--config", str(_small_config(tmp_path)), "--robots", "2", "--envs", "8", "--episodes", "1",
                       "--out", str(out), "--maps", "--plot"])
    text = capsys.readouterr().out
    lay = DeviceLayout(build_tables(evaluate_vec.build_spec(dict(width=36, height=30, exit_location=[36, 15]), 2)), 40)
    for name, policy in (("static", 4), ("random", "random")):
        maps = evaluate(lay, 8, 1, policy, metrics=True, timeline=True, maps=True)["maps"]
        z = np.load(out / f"maps_{name}.npz")
        assert sorted(z.files) == sorted(evaluate_vec.MAPS_KEYS)
        for k in su.MAPS + ("occupancy",):
            assert z[k].dtype == np.int64 and np.array_equal(z[k], maps["sum"][k]), (name, k)
        assert np.array_equal(z["density"], maps["sum"]["density"])
        assert np.array_equal(z["stall_ratio"], maps["sum"]["stall_ratio"], equal_nan=True)
        assert z["steps"] == maps["sum"]["steps"] and z["episodes"] == 8 and z["bad"] == 0
        assert z["exit_use"].shape[1] == 4 and z["exit_use"][:, 2].sum() == maps["sum"]["evac"].sum()
        assert z["hotspots"].tolist() == [list(h) for h in maps["sum"]["hotspots"]]
        assert evaluate_vec.maps_line(name, maps) in text and f"{name}: exit use (" in text
        assert "top stall cell (" in evaluate_vec.maps_line(name, maps)
        png = out / f"maps_{name}.png"
        assert png.exists() and png.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"


def test_evaluate_vec_without_maps_writes_none_of_it(tmp_path, capsys):
    _need_gpu()
    from Louvre_Evacuation.runners import evaluate_vec
    out = tmp_path / "out"
    evaluate_vec.main(["--config", str(_small_config(tmp_path)), "--robots", "2", "--envs", "8", "--episodes", "1",
                       "--out", str(out)])
    text = capsys.readouterr().out
    assert sorted(p.name for p in out.iterdir()) == ["strategy_comparison.csv"]
    assert "exit use" not in text and "maps_" not in text and "maps written" not in text


# ------------------------------------------------------------------ 7: refusals with live arrays
def test_a_refused_update_launches_nothing():
    _need_gpu()
    import ctypes
    from evacx import _lib
    from evacx.spatial import Grid, SpatialMaps
    E, P = 4, 10
    sm = SpatialMaps(E, "cuda", Grid(12, 9, P, 2))
    pk = torch.full((E * P,), 3 | (3 << 12), dtype=torch.int32, device="cuda")
    robots = torch.zeros(E * 2, dtype=torch.int32, device="cuda")
    done = torch.ones(E, dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    ok = (ctypes.byref(sm.c), pk.data_ptr(), robots.data_ptr(), done.data_ptr(), None, 0, None)
    for i, text in ((1, b"NULL pk or done"), (2, b"NULL robots with R > 0"), (3, b"NULL pk or done")):
        args = list(ok)
        args[i] = None
        assert L.evx_spatial_update(*args) == -22 and text in L.evx_spatial_last_error()
    for field, value, text in (("E", 0, b"E must be"), ("P", 16384, b"P must be"), ("GX", 4097, b"1..4096"),
                               ("GY", 0, b"1..4096"), ("n_rows", 0, b"n_rows"), ("arrive", None, b"NULL spatial buffer")):
        keep = getattr(sm.c, field)
        setattr(sm.c, field, value)
        assert L.evx_spatial_update(*ok) == -22 and text in L.evx_spatial_last_error()
        assert L.evx_spatial_sync(ctypes.byref(sm.c), pk.data_ptr(), None, None) == -22
        setattr(sm.c, field, keep)
    with pytest.raises(ValueError, match="done"):
        sm.update((pk, robots), done.to(torch.int32))
    got = _device_arrays(sm)
    assert all(not got[k].any() for k in got)  # nothing ran: prev, n_total and every map are as init left them
    sm.update((pk, robots), done)
    got = _device_arrays(sm)
    assert got["n_total"].tolist() == [1] * E and got["steps"][0] == E and got["robot"][0, 0, 0] == 2 * E
