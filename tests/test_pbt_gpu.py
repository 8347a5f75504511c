"""Population-based training on the GPU ("Exploit / explore"): evx_copy_members alone
against a host copy of the same blocks, ``PopulationTrainer.copy_members`` against ``copy_member``,
and ``evacx.pbt.PBTScheduler`` / ``train_pop --pbt-every`` driving a trainer -- all bit for bit
(torch.equal / numpy.array_equal). The trainers are tests/pop_util.py's small layout: K = 4, E = 8
(N = 8 rows per member and push), batch 256, ring 1024, so the first learn step is step 32."""
import csv
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pop_util as pu

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ 1. the kernel alone
KM = 6
SIZES = (4, 12, 16, 20, 4092, 4 * (4 * 1024 + 7))  # bytes per member: below, at and over 16; a ragged 16 KiB
MAPS = {"all from 0": [0, 0, 0, 0, 0, 0],  # dst - src = 1 .. 5
        "by four": [0, 1, 2, 3, 0, 1],  # dst - src = 4: the 16-byte path at every stride; 2 and 3 untouched
        "downwards": [4, 1, 4, 3, 4, 1]}  # dst - src = -4, -2, 4
GUARD_AFTER = 32  # bytes behind the last block


def _kernel_case(dtype):
    """24 arrays (every size x every stride residue mod 16) of one dtype, filled with random bits:
    [(device tensor, host copy, offset, stride, size)] in bytes. Member k's block starts offset + k
    stride bytes into its tensor; offset = 0, 4, 8 or 12 walks the blocks' alignment, so the 16-byte
    path runs with every head and tail length; at least 4 guard bytes lie between two blocks."""
    rng = np.random.default_rng(11)
    item = np.dtype(dtype).itemsize
    out = []
    for i, size in enumerate(SIZES):
        for j, res in enumerate((0, 4, 8, 12)):
            stride = size + 4 + (res - (size + 4)) % 16
            assert stride % 16 == res and stride >= size + 4
            off = 4 * ((i + j) % 4)
            total = off + KM * stride + GUARD_AFTER
            lim = np.iinfo(dtype)
            host = rng.integers(lim.min, lim.max, size=total // item, dtype=dtype, endpoint=True)
            out.append((torch.from_numpy(host.copy()).cuda(), host, off, stride, size))
    return out


def _call(case, src):
    from evacx import _lib
    from evacx.env import _stream
    bufs = (_lib.evx_member_buf * len(case))(*[
        _lib.evx_member_buf(base=t.data_ptr() + off, stride_bytes=stride, bytes=size) for t, _, off, stride, size in case])
    _lib.check(_lib.lib().evx_copy_members(bufs, len(case), (C.c_int32 * len(src))(*src), len(src), _stream()),
               "copy_members")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [np.int32, np.int16], ids=["int32", "int16"])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_copy_members_kernel_moves_the_blocks_and_nothing_else(name, dtype):
    """The whole backing array of every buffer against the host copy with the receivers' blocks
    replaced: receivers equal their donors' blocks, donors, untouched members and every guard byte
    between and behind the blocks keep their bits."""
    _need_gpu()
    src, case = MAPS[name], _kernel_case(dtype)
    for t, _, off, stride, _ in case:
        assert t.data_ptr() % 16 == 0  # so offset and stride alone decide the path
    paths = {(((off + k * stride) % 16 == (off + s * stride) % 16), (off + k * stride) % 16)
             for _, _, off, stride, _ in case for k, s in enumerate(src) if s != k}
    assert {p for p in paths if p[0]} == {(True, a) for a in (0, 4, 8, 12)} and (name == "by four") == \
        all(p[0] for p in paths)
    _call(case, src)
    for t, host, off, stride, size in case:
        orig = host.view(np.uint8)
        want = orig.copy()
        for k, s in enumerate(src):
            if s != k:
                want[off + k * stride:off + k * stride + size] = orig[off + s * stride:off + s * stride + size]
        got = t.cpu().numpy().view(np.uint8)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (size, stride, off, bad[:8].tolist())
        assert not np.array_equal(want, host.view(np.uint8))  # something did move


def test_copy_members_kernel_identity_map_changes_nothing():
    _need_gpu()
    case = _kernel_case(np.int32)
    _call(case, list(range(KM)))
    for t, host, *_ in case:
        assert np.array_equal(t.cpu().numpy(), host)


# ------------------------------------------------------------------ 2. copy_members against copy_member
K, E, B, CAP = 4, 8, 256, 1024
HP = dict(lr=(1e-3, 3e-4, 1e-4, 3e-3), gamma=(0.99, 0.95, 0.9, 0.97), epsilon=(1.0, 0.6, 0.3, 0.8), epsilon_min=0.02,
          epsilon_decay=(0.9, 0.8, 0.95, 0.85), target_every=(2, 3, 2, 3))
WARM = 36  # steps: learn steps at 32 .. 36 (t = 31 .. 35)
FLATS = ("flat", "tflat", "m", "v")


def _pop(**kw):
    from evacx.population import PopulationTrainer
    args = dict(HP)
    args.update(kw)
    return PopulationTrainer(pu.small_layout(), E, members=K, seed=5, batch=B, replay_capacity=CAP, **args)


def _state(tr):
    """name -> tensor of every buffer copy_members covers (4 flat arrays, 18 operand arrays)."""
    gl = tr.glearner
    out = {name: getattr(gl, name) for name in FLATS}
    for tag, fast in (("online", gl.fast), ("target", gl.fast_t)):
        assert sorted(fast.bufs) == sorted(pu.OPERANDS)
        out.update({f"{tag}.{name}": fast.bufs[name] for name in pu.OPERANDS})
    assert len(out) == 22
    return out


def _same(a, b, what, members=range(K)):
    sa, sb = _state(a), _state(b)
    for name in sa:
        for k in members:
            assert torch.equal(sa[name][k], sb[name][k]), (what, name, k)


def test_copy_members_equals_copy_member_calls():
    """Two equal trainers after 5 learn steps; the map [0, 0, 2, 2] as one copy_members launch on one
    and as copy_member(0, 1), copy_member(2, 3) -- tensor copies and repacks -- on the other: all 22
    buffers equal, so the copied operands are the bits a repack writes; after one more step of each,
    actions, losses and all 22 buffers still are."""
    _need_gpu()
    a, b = _pop(), _pop()
    for _ in range(WARM):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert a.learn_steps == b.learn_steps == WARM - B // a.N + 1 == 5
    _same(a, b, "before")
    before = {name: t.clone() for name, t in _state(a).items()}
    for name, t in before.items():  # the members differ, online and target too, so a copy is visible
        assert not torch.equal(t[0], t[1]) and not torch.equal(t[2], t[3]), name
    assert not torch.equal(a.glearner.flat, a.glearner.tflat)
    a.copy_members([0, 0, 2, 2])
    b.copy_member(0, 1)
    b.copy_member(2, 3)
    torch.cuda.synchronize()
    _same(a, b, "after the copy")
    for name, t in _state(a).items():
        assert torch.equal(t[1], before[name][0]) and torch.equal(t[3], before[name][2]), name
        assert torch.equal(t[0], before[name][0]) and torch.equal(t[2], before[name][2]), name
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.actions, b.actions) and torch.equal(a.last_loss, b.last_loss)
    _same(a, b, "one step later")
    assert not torch.equal(a.glearner.flat[1], a.glearner.flat[0])  # own envs, ring and lr: the copy moves on
    with pytest.raises(ValueError, match="itself replaced"):
        a.copy_members([0, 0, 1, 3])
    with pytest.raises(ValueError, match="4"):
        a.copy_members([0, 0, 2, 4])
    a.copy_members([0, 1, 2, 3])  # the identity map
    torch.cuda.synchronize()
    _same(a, b, "identity")


# ------------------------------------------------------------------ 3. a forced round
def _summary(returns, episodes=3):
    return {"per_member": [dict(episodes=episodes, return_sum=r * episodes, evacuated=0, dead=0) for r in returns]}


def test_forced_round_moves_the_worst_onto_the_best():
    _need_gpu()
    from evacx.pbt import PBTScheduler
    tr = _pop()
    for _ in range(WARM):
        tr.step()
    torch.cuda.synchronize()
    before = {name: t.clone() for name, t in _state(tr).items()}
    lr0 = list(tr.lr)
    s = PBTScheduler(K, {"lr": ("perturb", (0.8, 1.25), 1e-6, 1e-2)}, frac=0.25, seed=9)
    s.observe(_summary([9.0, 5.0, 4.0, -2.0]))
    d = s.round_(tr)
    torch.cuda.synchronize()
    assert [(x["dst"], x["src"], x["fitness_dst"], x["fitness_src"]) for x in d] == [(3, 0, -2.0, 9.0)]
    assert d[0]["old"] == {"lr": lr0[3]} and d[0]["new"] == {"lr": tr.lr[3]}
    assert tr.lr[3] in (lr0[0] * 0.8, lr0[0] * 1.25) and tr.lr[:3] == lr0[:3]
    assert tr.gamma == list(HP["gamma"]) and tr.epsilon[3] != tr.epsilon[0]  # not in the space: the receiver's own
    for name, t in _state(tr).items():
        assert torch.equal(t[3], before[name][0]), name
        for k in (0, 1, 2):
            assert torch.equal(t[k], before[name][k]), (name, k)
    assert s.round == 1 and s.plan(tr) == []  # the window was cleared


# ------------------------------------------------------------------ 4. off means off
ROUNDS_AT = (33, 35, 37)  # after learn steps 2, 4 and 6
SPACE = {"lr": ("perturb", (0.8, 1.25), 1e-6, 1e-2), "gamma": ("perturb", (0.98, 1.02), 0.5, 0.999),
         "target_every": ("resample", (1, 2, 4))}
_RUNS = {}


def _run(key, frac=None):
    """ROUNDS_AT[-1] + 1 steps of a trainer; at every step of ROUNDS_AT a scheduler (frac None: none)
    is fed a hand-made window -- episodes of the small layout take hundreds of steps -- that ranks the
    members differently each time, and runs a round. Returns (trainer, per-step actions, decisions)."""
    if key in _RUNS:
        return _RUNS[key]
    from evacx.pbt import PBTScheduler
    tr = _pop()
    s = None if frac is None else PBTScheduler(K, SPACE, frac=frac, seed=3)
    actions, decisions = [], []
    for step in range(1, ROUNDS_AT[-1] + 2):
        tr.step()
        actions.append(tr.actions.clone())
        if s is not None and step in ROUNDS_AT:
            s.observe(_summary([float((5 * k + 3 * s.round) % 7) for k in range(K)]))
            decisions.append(s.round_(tr))
    torch.cuda.synchronize()
    tr.env.check_err()
    _RUNS[key] = (tr, actions, decisions)
    return _RUNS[key]


def test_a_scheduler_that_replaces_nobody_changes_nothing():
    _need_gpu()
    plain, pa, _ = _run("plain")
    off, oa, od = _run("off", frac=0.0)
    assert od == [[], [], []]
    assert all(torch.equal(x, y) for x, y in zip(pa, oa))
    _same(plain, off, "frac 0")
    assert plain.lr == off.lr and plain.gamma == off.gamma and plain.target_every == off.target_every


def test_two_runs_with_rounds_are_bit_identical():
    _need_gpu()
    a, aa, ad = _run("pbt a", frac=0.25)
    b, ba, bd = _run("pbt b", frac=0.25)
    assert ad == bd and [len(d) for d in ad] == [1, 1, 1]
    assert len({(d[0]["dst"], d[0]["src"]) for d in ad}) > 1  # the hand-made windows rank differently
    assert all(torch.equal(x, y) for x, y in zip(aa, ba))
    _same(a, b, "two runs")
    assert a.lr == b.lr and a.gamma == b.gamma and a.target_every == b.target_every
    plain = _run("plain")[0]
    assert not torch.equal(plain.glearner.flat, a.glearner.flat) and plain.lr != a.lr  # the rounds did bear on it


# ------------------------------------------------------------------ 5. the runner
CFG = ("env:\n  width: 36\n  height: 30\n  fire_zones: [[18, 14]]\n  exit_location: [36, 15]\n  num_people: 40\n"
       "agent:\n  gamma: 0.99\n  epsilon: 1.0\n  epsilon_min: 0.02\n  epsilon_decay: 0.9995\n  learning_rate: 0.0001\n"
       "  batch_size: 32\n  target_update_freq: 20\n  memory_size: 1024\nsave_path: \"unused\"\n")


def test_train_pop_pbt_every_writes_pbt_log(tmp_path, monkeypatch, capsys):
    """train_pop at its smallest sizes: 4 members x 2 envs, 4 steps, a log line every 2 and a round
    at each. No episode ends that soon, so episode_summary is wrapped to report two finished episodes
    per member and window, member k's return k + 1: member 0 takes from member 3 in both rounds.
    pbt_log.csv has the header and one row per decision; without --pbt-every it is not written."""
    _need_gpu()
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(pu.__file__)), "..", "dqn-marl_amd"))
    from Louvre_Evacuation.runners import train_pop
    from evacx.population import PopulationTrainer
    real = PopulationTrainer.episode_summary

    def two_episodes_each(self, clear=True):
        out = real(self, clear=clear)
        for k, row in enumerate(out["per_member"]):
            row.update(episodes=2, return_sum=2.0 * (k + 1), return_mean=float(k + 1), return_std=0.0, length_mean=9.0,
                       evacuated=40 + k, dead=4 - k, evac_rate=(40 + k) / 80, death_rate=(4 - k) / 80)
        return out
    monkeypatch.setattr(PopulationTrainer, "episode_summary", two_episodes_each)
    cfg = tmp_path / "small.yaml"
    cfg.write_text(CFG)
    common = ["--config", str(cfg), "--members", "4", "--envs", "8", "--log-every", "2", "--lr", "1e-3,3e-4,1e-4,3e-5",
              "--batch", "16"]
    out = tmp_path / "pbt"
    tr = train_pop.main(common + ["--steps", "4", "--out", str(out), "--pbt-every", "2", "--pbt-frac", "0.25",
                                  "--pbt-space", "lr:perturb:0.8,1.25:1e-6:1e-2;target_every:resample:5,10"])
    printed = capsys.readouterr().out
    rows = list(csv.reader(open(out / "pbt_log.csv")))
    assert rows[0] == train_pop.PBT_COLUMNS + ["lr_old", "lr_new", "target_every_old", "target_every_new"]
    rounds = re.findall(r"^pbt round (\d+) at step (\d+): (.*)$", printed, flags=re.M)
    assert [(r, s) for r, s, _ in rounds] == [("0", "2"), ("1", "4")]
    assert len(rows) - 1 == sum(text.count(" <- ") for _, _, text in rounds) == 2
    col = {name: i for i, name in enumerate(rows[0])}
    lr = 3e-5
    for i, row in enumerate(rows[1:]):
        assert [row[col[c]] for c in ("round", "step", "dst", "src")] == [str(i), str(2 * i + 2), "0", "3"]
        assert (float(row[col["fitness_dst"]]), float(row[col["fitness_src"]])) == (1.0, 4.0)
        assert float(row[col["lr_new"]]) in (lr * 0.8, lr * 1.25) and row[col["target_every_new"]] in ("5", "10")
    assert float(rows[1][col["lr_old"]]) == 1e-3 and rows[2][col["lr_old"]] == rows[1][col["lr_new"]]
    assert tr.lr[0] == float(rows[2][col["lr_new"]]) and tr.target_every[0] == int(rows[2][col["target_every_new"]])
    assert tr.lr[1:] == [3e-4, 1e-4, 3e-5]
    assert torch.equal(tr.glearner.flat[0], tr.glearner.flat[3])  # (the last round ends the run)
    for name in ("population_summary.csv", "best_member.json", os.path.join("member0", "training_log.csv")):
        assert (out / name).exists(), name
    summ = list(csv.reader(open(out / "population_summary.csv")))
    assert summ[0] == train_pop.SUMMARY_COLUMNS and [r[0] for r in summ[1:]] == ["2", "4"]
    plain = tmp_path / "plain"
    train_pop.main(common + ["--steps", "2", "--out", str(plain)])
    assert (plain / "population_summary.csv").exists() and not (plain / "pbt_log.csv").exists()
    assert "pbt round" not in capsys.readouterr().out
