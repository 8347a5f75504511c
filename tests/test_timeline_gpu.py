"""Evacuation timelines on the device (csrc/timeline.hip, evacx.timeline), evaluate(timeline=True)
and the runner's --curves / --track.

The reference everywhere is timeline_util.timeline_ref, the update restated in numpy and fed from
the host -- the fixtures' own records, seeded arrays, or the state read back from a second VecEnv
-- never the Timeline itself. Every array is compared bit for bit."""
import csv

import numpy as np
import pytest
import torch

import timeline_util as tu

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
PAD = 64  # sentinel bytes * 8 behind every array


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if want.dtype == np.float64:
        return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))
    return got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64))


def _device_arrays(tl):
    names = ["t", "p_evac", "p_dead", "n_total", *tu.SLOTS, "late", "bad_health"]
    if tl.n_trk:
        names += ["trk_pk", "trk_health", "trk_len"]
    torch.cuda.synchronize()
    out = {k: getattr(tl, k).cpu().numpy() for k in names}
    if tl.n_trk:
        out["trk_pk"] = out["trk_pk"].view(np.uint32)
    return out


def _assert_equals_ref(tl, ref, skip=()):
    got, want = _device_arrays(tl), ref.arrays()
    assert sorted(got) == sorted(want)
    for k in want:
        if k not in skip:
            assert _same(got[k], want[k]), (k, got[k], want[k])
    return got


# ------------------------------------------------------------------ 1: the reference trajectories
@pytest.mark.parametrize("name", ["cfg1_single_traj", "cfg1_multi_traj"])
def test_replayed_reference_trajectory_gives_the_fixture_timeline(name):
    _need_gpu()
    from golden_util import traj_tables
    from evacx.env import DeviceLayout, VecEnv
    from evacx.timeline import Timeline
    tr, pk, eps = tu.fixture(name)
    tables, P = traj_tables(name)
    T, everyone = 96, ([0] * P, list(range(P)))
    env = VecEnv(DeviceLayout(tables, P), 1)
    tl = Timeline(1, "cuda", P, T=T, track=everyone)
    ref = tu.timeline_ref(1, P, T, track=everyone)
    for k in range(len(tr["done"])):
        if tr["is_reset"][k]:
            if k == 0:
                env.set_rng(tr["rng_py"][0][None], tr["rng_np"][0][None])
            env.reset()
            if k == 0:
                tl.trace0(env)
                ref.trace0(pk[0], tr["snap_health"][0])
            continue
        env.step(torch.from_numpy(tr["actions"][k].astype(np.int32)).cuda())
        tl.update(env, env.done, env.counts)
        ref.update([[tr["evac"][k], tr["dead"][k]]], [tr["done"][k]], pk[k], tr["snap_health"][k])
    env.check_err()
    got = _assert_equals_ref(tl, ref, skip=("trk_pk",))
    assert got["n_total"][0] == len(eps) and got["seen"][0, 0] == len(eps) and not got["late"].any()
    # the trace is the fixture's snapshot of the first episode, slot 0 = the reset row
    n = eps[0][1] + 1
    assert (got["trk_len"] == n).all()
    word = got["trk_pk"][:n]
    assert np.array_equal(word & 0xFFF, tr["snap_pos"][:n, :, 0]) and np.array_equal((word >> 12) & 0xFFF,
                                                                                     tr["snap_pos"][:n, :, 1])
    assert np.array_equal((word >> 24) & 3, tr["snap_flags"][:n])
    assert _same(got["trk_health"][:n], tr["snap_health"][:n])
    assert not got["trk_pk"][n:].any() and not got["trk_health"][n:].any()  # later episodes are not traced
    cv = tl.curves()
    assert cv["episodes"] == len(eps) and cv["tracked"]["len"].tolist() == [n] * P
    assert (cv["tracked"]["evac_step"] >= 0).sum() == tr["evac"][eps[0][1]]
    assert cv["new_evacuated"].sum() == sum(tr["evac"][b] for _, b in eps)


# ------------------------------------------------------------------ 2-4: synthetic, no env
def _synthetic(P, E=37, steps=12, seed=0):
    """Per step (counts [E, 2], done [E], pk [E, P], health [E, P]): counts grow within an episode and
    start again after done; env 0 never finishes, so its episode runs past T."""
    rng = np.random.default_rng(1000 * seed + P)
    ev, dd = np.zeros(E, np.int64), np.zeros(E, np.int64)
    out = []
    for s in range(steps):
        ev += rng.integers(0, 3, E)
        dd += rng.integers(0, 2, E)
        done = (rng.random(E) < 0.3).astype(np.uint8)
        done[0] = 0
        health = rng.random((E, P)) * 100
        health[rng.random((E, P)) < 0.05] = 0.0
        dead = rng.random((E, P)) < rng.random((E, 1))
        word = rng.integers(1, 60, (E, P)) | (rng.integers(1, 60, (E, P)) << 12) | \
            np.where(rng.random((E, P)) < 0.2, tu.SAFE, 0) | np.where(dead, tu.DEAD, 0)
        if s == 0:  # one person far out of range, not dead: counted in bad_health and in no sum
            health[0, 0] = 1e6
            word[0, 0] &= ~tu.DEAD
        out.append((np.stack([ev, dd], 1).astype(np.int32), done, word.astype(np.uint32).view(np.int32), health))
        ev[done != 0] = 0
        dd[done != 0] = 0
    return out


def _padded(tl):
    """Every array of the Timeline moved in front of sentinel words; returns the backing buffers."""
    from evacx import _lib
    backing = {}
    names = ["t", "p_evac", "p_dead", "n_total", *tu.SLOTS, "late", "bad_health"]
    if tl.n_trk:
        names += ["trk_env", "trk_person", "trk_pk", "trk_health", "trk_len"]
    for k in names:
        old = getattr(tl, k)
        nbytes = old.numel() * old.element_size()
        buf = torch.full((nbytes + PAD * 8,), SENTINEL, dtype=torch.uint8, device=old.device)
        new = buf[:nbytes].view(old.dtype).view(old.shape)
        new.copy_(old)
        setattr(tl, k, new)
        setattr(tl.c, k, new.data_ptr())
        backing[k] = (buf, nbytes)
    import ctypes
    _lib.check(_lib.lib().evx_timeline_init(ctypes.byref(tl.c), None), "timeline_init")
    return backing


def _run_synthetic(P, with_state=True, track=True):
    from evacx.timeline import Timeline
    E, T, cap = 37, 8, 2
    lidx = (np.arange(E) % 3).astype(np.int32)
    trk = ([0, 5, 36, 36], [0, P - 1, 3 % P, 0]) if track else None
    tl = Timeline(E, "cuda", P, T=T, layout_idx=torch.from_numpy(lidx).cuda(), n_layouts=3, cap=cap, track=trk)
    backing = _padded(tl)
    ref = tu.timeline_ref(E, P, T, n_rows=3, layout_idx=lidx, cap=cap, track=trk)
    data = _synthetic(P)
    if track:
        tl.trace0((torch.from_numpy(data[0][2]).cuda().view(-1), torch.from_numpy(data[0][3]).cuda().view(-1)))
        ref.trace0(data[0][2], data[0][3])
    for counts, done, word, health in data:
        state = (torch.from_numpy(word).cuda().view(-1), torch.from_numpy(health).cuda().view(-1))
        tl.update(state if with_state else None, torch.from_numpy(done).cuda(),
                  torch.from_numpy(counts).cuda().view(-1))
        ref.update(counts, done, word if with_state else None, health if with_state else None)
    torch.cuda.synchronize()
    for k, (buf, nbytes) in backing.items():
        assert (buf[nbytes:] == SENTINEL).all().item(), f"{k}: written past its end"
    return tl, ref


@pytest.mark.parametrize("P", [7, 64, 65, 569])
def test_synthetic_steps_equal_the_numpy_restatement_and_repeat(P):
    _need_gpu()
    tl, ref = _run_synthetic(P)
    got = _assert_equals_ref(tl, ref)
    assert got["bad_health"][0] == 1
    assert got["late"][0, 3] >= 4  # env 0 (row 0) never finishes: its steps 9..12 are late
    assert (got["n_total"] > 2).any() and (got["seen"][:, 0].sum() <= 2 * 37)  # the cap kept later episodes out
    assert got["alive"].sum() > 0 and (got["trk_len"] >= 1).all()
    # the out-of-range person is in no sum: the same run without it differs in that slot by nothing else
    slot0 = ref.health_q[0, 0]
    assert got["health_q"][0, 0] == slot0 and slot0 < 37 * P * 100 * 2 ** 20
    tl2, _ = _run_synthetic(P)
    again = _device_arrays(tl2)
    for k in got:
        assert _same(again[k], got[k]), k


def test_contention_on_one_slot_adds_up_exactly():
    _need_gpu()
    from evacx.timeline import Timeline
    E, P, T = 2048, 16, 4
    rng = np.random.default_rng(9)
    tl = Timeline(E, "cuda", P, T=T)
    want = {k: np.zeros(T, np.int64) for k in tu.SLOTS}
    prev = np.zeros((E, 2), np.int64)
    for s in range(3):  # nobody finishes: every env is on slot s
        counts = prev + rng.integers(0, 4, (E, 2))
        health = rng.random((E, P)) * 100
        dead = rng.random((E, P)) < 0.3
        word = np.where(dead, tu.DEAD, 0).astype(np.uint32).view(np.int32)
        tl.update((torch.from_numpy(word).cuda().view(-1), torch.from_numpy(health).cuda().view(-1)),
                  torch.zeros(E, dtype=torch.uint8, device="cuda"),
                  torch.from_numpy(counts.astype(np.int32)).cuda().view(-1))
        want["evac"][s], want["dead"][s] = (counts - prev).sum(axis=0)
        want["seen"][s] = E
        want["alive"][s] = int((~dead).sum())
        want["health_q"][s] = int(np.rint(health[~dead] * 2 ** 20).astype(np.int64).sum())
        prev = counts
    got = _device_arrays(tl)
    for k in tu.SLOTS:
        assert _same(got[k][0], want[k]), (k, got[k], want[k])
    assert (got["t"] == 3).all() and not got["late"].any() and got["bad_health"][0] == 0
    assert _same(got["p_evac"], prev[:, 0]) and _same(got["p_dead"], prev[:, 1])


def test_without_the_state_only_the_health_fields_stay_empty():
    _need_gpu()
    P = 65
    tl, ref = _run_synthetic(P, with_state=False, track=False)
    got = _assert_equals_ref(tl, ref)
    assert not got["alive"].any() and not got["health_q"].any() and got["bad_health"][0] == 0
    full = _device_arrays(_run_synthetic(P, track=False)[0])
    for k in ("t", "p_evac", "p_dead", "n_total", "evac", "dead", "ended", "seen", "late"):
        assert _same(got[k], full[k]), k
    assert full["alive"].any()


# ------------------------------------------------------------------ 5: evaluate(timeline=True)
def _cfg1_layout():
    from golden_util import traj_tables
    from evacx.env import DeviceLayout
    tables, P = traj_tables("cfg1_single_traj")
    return DeviceLayout(tables, P), P


def test_evaluate_with_the_timeline_leaves_the_trajectory_alone_and_matches_a_host_loop():
    _need_gpu()
    from evacx.env import VecEnv
    from evacx.evaluate import evaluate
    lay, P = _cfg1_layout()
    E, K, action = 16, 2, 4
    trk = ([0, 0, 3, 15], [0, 149, 7, 20])
    off = evaluate(lay, E, K, action)
    on = evaluate(lay, E, K, action, timeline=True, track=trk)
    assert set(on) - set(off) == {"curves"}
    for k in off:
        if k == "per_env":
            for name, x in off[k].items():
                y = on[k][name]
                assert torch.equal(x.view(torch.int64), y.view(torch.int64)) if x.dtype == torch.float64 \
                    else torch.equal(x, y), name
        else:
            assert off[k] == on[k], k
    cv = on["curves"]
    n = E * K
    print(f"steps {on['steps']}, episodes {on['episodes']}, evacuated {on['evacuated']}, dead {on['dead']}, "
          f"last step with an episode running {int(np.nonzero(cv['running'])[0][-1]) + 1}")
    assert on["episodes"] == n == cv["episodes"] and cv["bad_health"] == 0
    assert cv["new_evacuated"].sum() + cv["late"][0] == on["evacuated"]
    assert cv["new_dead"].sum() + cv["late"][1] == on["dead"]
    assert cv["ended"].sum() + cv["late"][2] == n and not cv["late"].any()
    before = np.concatenate([[0], np.cumsum(cv["ended"])[:-1]])
    assert np.array_equal(cv["running"], n - before)
    assert cv["evacuated_mean"][-1] == on["evacuated"] / n and cv["dead_mean"][-1] == on["dead"] / n
    # the host loop: a second VecEnv, its outputs and state read back every step
    env = VecEnv(lay, E)
    env.seed([1234 + i for i in range(E)])
    env.reset()
    ref = tu.timeline_ref(E, P, 1200, cap=K, track=trk)
    ref.trace0(env.pk.cpu().numpy(), env.health.cpu().numpy())
    a = torch.full((E * lay.R,), action, dtype=torch.int32, device="cuda")
    for _ in range(on["steps"]):
        env.step(a, auto_reset=False)
        ref.update(env.counts.cpu().numpy().reshape(E, 2), env.done.cpu().numpy(), env.pk.cpu().numpy(),
                   env.health.cpu().numpy())
        env.reset(mask=env.done)
    env.check_err()
    for k, name in (("evac", "new_evacuated"), ("dead", "new_dead"), ("ended", "ended"), ("seen", "running"),
                    ("alive", "alive")):
        assert _same(cv[name], getattr(ref, k)[0]), k
        assert _same(cv["per_layout"][0][name], getattr(ref, k)[0]), k
    alive, hq = ref.alive[0], ref.health_q[0]
    with np.errstate(all="ignore"):
        want = np.where(alive > 0, hq / 2.0 ** 20 / np.where(alive > 0, alive, 1), np.nan)
    assert np.array_equal(np.isnan(cv["avg_health"]), np.isnan(want))
    assert _same(cv["avg_health"][alive > 0], want[alive > 0])
    t = cv["tracked"]
    assert t["env"].tolist() == trk[0] and t["person"].tolist() == trk[1]
    assert _same(t["len"], ref.trk_len) and _same(t["health"], ref.trk_health)
    assert np.array_equal(t["x"], ref.trk_pk & 0xFFF) and np.array_equal(t["dead"], (ref.trk_pk & tu.DEAD) != 0)
    # with the health metrics as well: the same curves, the same health table
    both = evaluate(lay, E, K, action, metrics=True, timeline=True)
    assert _same(both["curves"]["new_evacuated"], cv["new_evacuated"])
    assert _same(both["curves"]["avg_health"][alive > 0], want[alive > 0])
    assert "tracked" not in both["curves"] and both["avg_health"] is not None
    with pytest.raises(ValueError, match="track needs timeline"):
        evaluate(lay, E, K, action, track=5)


# ------------------------------------------------------------------ 6: the runner
def test_evaluate_vec_writes_the_curves_and_the_tracked_persons(tmp_path, capsys):
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.evaluate import evaluate
    from evacx.layout import build_tables
    from Louvre_Evacuation.runners import evaluate_vec
    cfg = tmp_path / "small.yaml"
    cfg.write_text("env:\n  width: 36\n  height: 30\n  fire_zones: [[18, 14]]\n  exit_location: [36, 15]\n"
                   "  num_people: 40\nagent:\n  gamma: 0.99\nsave_path: \"unused\"\n")
    out = tmp_path / "out"
    evaluate_vec.main(["--config", str(cfg), "--robots", "2", "--envs", "8", "--episodes", "1", "--out", str(out),
                       "--curves", "--track", "5"])
    text = capsys.readouterr().out
    assert "curves_static.csv" in text and "tracked_random.npz" in text
    assert not list(out.glob("*.png"))  # no --plot
    lay = DeviceLayout(build_tables(evaluate_vec.build_spec(dict(width=36, height=30, exit_location=[36, 15]), 2)), 40)
    for name, policy in (("static", 4), ("random", "random")):
        cv = evaluate(lay, 8, 1, policy, metrics=True, timeline=True, track=5)["curves"]
        rows = list(csv.reader(open(out / f"curves_{name}.csv")))
        steps = int(np.nonzero(cv["running"])[0][-1]) + 1
        assert rows[0] == evaluate_vec.CURVE_COLUMNS and len(rows) == steps + 1
        for s, row in enumerate(rows[1:]):
            for k, v in zip(evaluate_vec.CURVE_COLUMNS, row):
                want = cv[k][s]
                assert (v == "" and np.isnan(want)) or float(v) == want, (name, s, k, v, want)
        z = np.load(out / f"tracked_{name}.npz")
        assert sorted(z.files) == sorted(cv["tracked"])
        for k in z.files:
            assert _same(z[k], cv["tracked"][k]), (name, k)
        assert z["person"].tolist() == [0, 1, 2, 3, 4] and (z["len"] >= 2).all()
