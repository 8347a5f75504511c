"""Learner diagnostics without a device: the library's entries and descriptors, their refusals, the
front ends' argument checks, the runner's flag, and the numpy restatements (tests/lstats_util.py)
that tests/test_lstats_gpu.py holds the kernels to, pinned on hand-made cases."""
import ctypes
import math
import os

import numpy as np
import pytest

import lstats_util as lu

ENTRIES = ("evx_lstats_ws_doubles", "evx_lstats_init", "evx_lstats_update", "evx_lstats_last_error",
           "evx_vprobe_init", "evx_vprobe_update", "evx_vprobe_discard", "evx_vprobe_reduce")
F32 = np.float32


# ------------------------------------------------------------------ the C entries, no device
def test_library_exports_the_entries_and_both_descriptors_mirror_the_header(tmp_path):
    import shutil
    import subprocess
    from golden_util import ROOT
    from evacx import _lib
    L = _lib.lib()
    for s in ENTRIES:
        assert hasattr(L, s) and s in _lib.SIGNATURES, s
    vp = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.evx_lstats) == 8 + 23 * vp and ctypes.sizeof(_lib.evx_vprobe) == 16 + 16 * vp
    consts = {"EVX_LSTATS_MAX_A": _lib.LSTATS_MAX_A, "EVX_LSTATS_TD_BUCKETS": _lib.LSTATS_TD_BUCKETS,
              "EVX_LSTATS_WS_FIELDS": _lib.LSTATS_WS_FIELDS, "sizeof(evx_vprobe_row)": 8 * _lib.VPROBE_ROW_WORDS}
    assert (lu.MAX_A, lu.TD_BUCKETS, lu.SPAN) == (_lib.LSTATS_MAX_A, _lib.LSTATS_TD_BUCKETS, _lib.EPISODE_REDUCE_SPAN)
    cc = shutil.which("cc") or shutil.which("clang") or shutil.which("clang", path="/opt/rocm/llvm/bin")
    assert cc, "no C compiler (cc, clang) to check the structure layouts with"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "evacx.h"', "int main(void) {"]
    want = []
    for name in ("evx_lstats", "evx_vprobe"):
        S = getattr(_lib, name)
        lines.append(f'    printf("%d\\n", (int)sizeof({name}));')
        lines += [f'    printf("%d\\n", (int)offsetof({name}, {f}));' for f, _ in S._fields_]
        want += [ctypes.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    for expr, value in consts.items():
        lines.append(f'    printf("%d\\n", (int)({expr}));')
        want.append(value)
    row = ("probes", "bad", "open", "q_sum", "g_sum", "e_sum", "e2_sum", "q2_sum", "g2_sum", "qg_sum", "e_min", "e_max")
    lines += [f'    printf("%d\\n", (int)offsetof(evx_vprobe_row, {f}));' for f in row]
    want += [8 * k for k in range(len(row))]
    src, exe = tmp_path / "ls.c", tmp_path / "ls"
    src.write_text("\n".join(lines + ["    return 0;", "}"]) + "\n")
    r = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def _host(struct, leave_out=None, **ints):
    """A descriptor whose pointers are host scratch: only ever passed to calls that must fail before
    they launch anything."""
    keep, d = [], struct(**ints)
    for name, t in struct._fields_:
        if t is not ctypes.c_void_p or name == leave_out:
            continue
        buf = (ctypes.c_int64 * 64)()
        keep.append(buf)
        setattr(d, name, ctypes.addressof(buf))
    return d, keep


def test_lstats_entries_refuse_before_any_launch():
    from evacx import _lib
    L = _lib.lib()
    err, ref = L.evx_lstats_last_error, ctypes.byref
    bufs = [(ctypes.c_int64 * 64)() for _ in range(6)]

    def upd(d, Q=bufs[0], Qt=bufs[1], act=bufs[2], rew=bufs[3], done=bufs[4], gamma=0.99, B=4, ws=bufs[5], wsn=64):
        return L.evx_lstats_update(None if d is None else ref(d), Q, Qt, act, rew, done, gamma, B, None, None, None,
                                   1.0, None, ws, wsn, None)
    assert _lib.lib().evx_lstats_ws_doubles(257, 3) == 3 * 2 * 10 and L.evx_lstats_ws_doubles(0, 3) == 0
    assert upd(None) == -22 and b"lstats_update: NULL statistics descriptor" in err()
    assert L.evx_lstats_init(None, None) == -22 and b"lstats_init: NULL statistics descriptor" in err()
    assert err() == L.evx_last_error()  # the one thread-local error text
    for name in ("steps", "rows_bad", "act_hist", "td_hist", "s_q", "s_norm", "min_q", "max_norm"):
        d, keep = _host(_lib.evx_lstats, leave_out=name, nets=1, A=5)
        assert upd(d) == -22 and b"lstats_update: NULL statistics buffer" in err(), name
        assert L.evx_lstats_init(ref(d), None) == -22 and b"lstats_init: NULL statistics buffer" in err()
    d, keep = _host(_lib.evx_lstats, nets=1, A=5)
    for nets in (0, -1, 65):
        d.nets = nets
        assert upd(d) == -22 and b"nets must be 1..64" in err(), nets
        assert L.evx_lstats_init(ref(d), None) == -22 and b"nets must be 1..64" in err()
    d.nets = 1
    for A in (0, -2, 9):
        d.A = A
        assert upd(d) == -22 and b"A must be 1..8" in err(), A
    d.A = 5
    for k in ("Q", "Qt", "act", "rew", "done"):
        assert upd(d, **{k: None}) == -22 and b"NULL Q, Qt, act, rew or done" in err(), k
    for B in (0, -5):
        assert upd(d, B=B) == -22 and b"B must be >= 1" in err()
    for g in (math.nan, math.inf, -math.inf):
        assert upd(d, gamma=g) == -22 and b"gamma is not finite" in err()
    assert upd(d, ws=None) == -22 and b"NULL workspace" in err()
    assert upd(d, B=257, wsn=19) == -22 and b"workspace smaller" in err()
    d.nets = 64
    assert upd(d, B=1 << 26) == -22 and b"beyond 2^31 - 1" in err()
    assert err() == L.evx_last_error()


def test_vprobe_entries_refuse_before_any_launch():
    from evacx import _lib
    L = _lib.lib()
    err, ref = L.evx_lstats_last_error, ctypes.byref
    bufs = [(ctypes.c_int64 * 64)() for _ in range(5)]

    def upd(d, Q=bufs[0], act=bufs[1], reward=bufs[2], done=bufs[3], gamma=0.99):
        return L.evx_vprobe_update(None if d is None else ref(d), Q, act, reward, done, gamma, None)
    assert upd(None) == -22 and b"vprobe_update: NULL probe descriptor" in err()
    assert L.evx_vprobe_init(None, None) == -22 and b"vprobe_init: NULL probe descriptor" in err()
    assert L.evx_vprobe_discard(None, None, None) == -22 and b"vprobe_discard: NULL probe descriptor" in err()
    assert L.evx_vprobe_reduce(None, None, 1, bufs[4], 0, None) == -22 and b"vprobe_reduce: NULL probe" in err()
    assert err() == L.evx_last_error()
    for name in ("open", "q0", "len", "w_n", "w_bad", "w_qg", "w_emax"):
        d, keep = _host(_lib.evx_vprobe, leave_out=name, E=4, R=2, A=5)
        assert upd(d) == -22 and b"vprobe_update: NULL probe buffer" in err(), name
        assert L.evx_vprobe_init(ref(d), None) == -22 and L.evx_vprobe_discard(ref(d), None, None) == -22
        assert L.evx_vprobe_reduce(ref(d), None, 1, bufs[4], 0, None) == -22 and b"NULL probe buffer" in err()
    d, keep = _host(_lib.evx_vprobe, E=4, R=2, A=5)
    for E, R, A in ((0, 2, 5), (-1, 2, 5), (4, 0, 5), (4, 2, 0)):
        d.E, d.R, d.A = E, R, A
        assert upd(d) == -22 and b"E, R and A must be >= 1" in err(), (E, R, A)
        assert L.evx_vprobe_init(ref(d), None) == -22 and b"E, R and A must be >= 1" in err()
    d.E, d.R, d.A = 4, 2, 9
    assert upd(d) == -22 and b"A must be <= 8" in err()
    d.A = 5
    for k in ("Q", "act", "reward", "done"):
        assert upd(d, **{k: None}) == -22 and b"NULL Q, act, reward or done" in err(), k
    for g in (math.nan, math.inf, -0.01, 1.0000001):
        assert upd(d, gamma=g) == -22 and b"gamma must be in [0, 1]" in err(), g
    assert L.evx_vprobe_reduce(ref(d), None, 1, None, 0, None) == -22 and b"NULL output rows" in err()
    assert L.evx_vprobe_reduce(ref(d), None, 0, bufs[4], 0, None) == -22 and b"n_layouts must be 1..65535" in err()
    assert L.evx_vprobe_reduce(ref(d), None, 2, bufs[4], 0, None) == -22 and b"need layout_idx" in err()


# ------------------------------------------------------------------ the front ends
def test_front_ends_check_their_arguments_before_the_device():
    import torch
    from evacx.lstats import LearnStats, ValueProbe, _ProbeSlice
    for bad in (dict(nets=0), dict(nets=65), dict(nets=1, A=0), dict(nets=1, A=9)):
        with pytest.raises(ValueError):
            LearnStats(bad.pop("nets"), "cuda", **bad)
    for bad in (dict(E=0, R=2), dict(E=4, R=0), dict(E=4, R=2, A=9), dict(E=4, R=2, gamma=1.5),
                dict(E=4, R=2, gamma=math.nan), dict(E=4, R=2, n_layouts=0), dict(E=4, R=2, n_layouts=2),
                dict(E=4, R=2, n_layouts=2, layout_idx=torch.zeros(3, dtype=torch.int32))):
        bad.setdefault("gamma", 0.99)
        with pytest.raises(ValueError):
            ValueProbe(bad.pop("E"), bad.pop("R"), "cuda", **bad)
    # update's checks run before the library is called: an object without device arrays shows them
    ls = object.__new__(LearnStats)
    ls.nets, ls.A, ls.device = 2, 5, torch.device("cpu")
    B = 4
    ok = dict(Q=torch.zeros(2 * B, 5), Qt=torch.zeros(2 * B, 5), a=torch.zeros(2 * B, dtype=torch.int32),
              r=torch.zeros(2 * B), done=torch.zeros(2 * B, dtype=torch.uint8))
    for key, wrong in (("Q", torch.zeros(2 * B, 5, dtype=torch.float64)), ("Q", torch.zeros(2 * B, 4)),
                       ("Qt", torch.zeros(B, 5)), ("a", torch.zeros(2 * B, dtype=torch.int64)),
                       ("r", torch.zeros(2 * B, dtype=torch.float64)), ("done", torch.zeros(2 * B, dtype=torch.bool)),
                       ("done", torch.zeros(2 * B + 1, dtype=torch.uint8)), ("r", [0.0] * (2 * B)),
                       ("Q", torch.zeros(2 * B, 5, device="meta"))):
        with pytest.raises(ValueError, match=key):
            ls.update(**dict(ok, **{key: wrong}), gamma=0.99, B=B)
    for key, wrong in (("sel", torch.zeros(2 * B, dtype=torch.int64)), ("gamma_row", torch.zeros(B)),
                       ("loss", torch.zeros(1)), ("norm", torch.zeros(2, dtype=torch.float64)),
                       ("d_out", torch.zeros(2 * B, 2))):
        with pytest.raises(ValueError, match=key):
            ls.update(**ok, gamma=0.99, B=B, **{key: wrong})
    with pytest.raises(ValueError, match="B must be"):
        ls.update(**ok, gamma=0.99, B=0)
    with pytest.raises(ValueError, match="gamma"):
        ls.update(**ok, gamma=math.inf, B=B)
    vp = object.__new__(_ProbeSlice)
    vp.owner = type("O", (), dict(R=2, A=5, device=torch.device("cpu"), gamma=0.99))()
    vp.E = 3
    okp = dict(Q=torch.zeros(6, 5), act=torch.zeros(6, dtype=torch.int32), reward=torch.zeros(3, dtype=torch.float64),
               done=torch.zeros(3, dtype=torch.uint8))
    for key, wrong in (("Q", torch.zeros(6, 4)), ("Q", torch.zeros(6, 5, dtype=torch.float16)),
                       ("act", torch.zeros(3, dtype=torch.int32)), ("reward", torch.zeros(3)),
                       ("done", torch.zeros(3, dtype=torch.int32)),
                       ("done", torch.zeros(3, dtype=torch.uint8, device="meta"))):
        with pytest.raises(ValueError, match=key):
            vp.update(**dict(okp, **{key: wrong}))
    with pytest.raises(ValueError, match="mask"):
        vp.discard(torch.zeros(4, dtype=torch.uint8))


def test_learners_refuse_statistics_of_another_shape():
    from evacx.lstats import LearnStats
    from evacx.qgroup import GroupedLearner
    from evacx.qnet import Learner
    ls = object.__new__(LearnStats)
    ls.nets, ls.A = 2, 5
    with pytest.raises(ValueError, match="LearnStats of 1 net"):
        Learner(stats=ls)
    with pytest.raises(ValueError, match="LearnStats of 3 nets"):
        GroupedLearner(3, stats=ls)


def test_runner_takes_the_flag_and_the_trainer_refuses_qmix_statistics():
    from Louvre_Evacuation.runners import train_vec
    from evacx.trainer import VecTrainer
    assert train_vec.parse_args([]).learn_stats is False
    assert train_vec.parse_args(["--learn-stats"]).learn_stats is True
    assert train_vec.LEARN_COLUMNS == [
        "step", "learn_steps", "q_mean", "qmax_mean", "target_mean", "td_abs_mean", "td_rms", "td_p50", "td_p90",
        "td_p99", "td_abs_max", "greedy_frac", "grad_norm_mean", "grad_norm_max", "clipped_frac", "rows_bad",
        "steps_bad", "probes", "q0_mean", "return_mean", "bias", "rmse", "corr"]
    ls = dict({k: 1.5 for k in train_vec.LEARN_COLUMNS[2:15]}, rows_bad=2, steps_bad=0, td_p99=None)
    vs = dict(probes=7, q0_mean=1.0, return_mean=2.0, bias=-1.0, rmse=1.0, corr=None)
    row = train_vec.learn_row(300, 299, ls, vs)
    assert len(row) == len(train_vec.LEARN_COLUMNS) and row[:3] == [300, 299, "1.5"]
    assert row[9] == "" and row[15:18] == ["2", "0", "7"] and row[-1] == "" and row[-3] == "-1.0"
    with pytest.raises(ValueError, match="learn_stats"):  # before anything touches the device
        VecTrainer(None, 64, nets="qmix", learn_stats=True)


# ------------------------------------------------------------------ the restatements themselves
def test_bucket_edges():
    below = np.nextafter(F32(2.0 ** -23), F32(0))
    vals = np.array([0.0, 2.0 ** -23, below, 1.0, np.nextafter(F32(2.0), F32(0)), 2.0 ** 23, 2.0 ** -24, 2.0 ** -22,
                     2.0 ** 22, 3e38, 1e-45], F32)
    assert lu.bucket(vals).tolist() == [0, 1, 0, 24, 24, 47, 0, 2, 46, 47, 0]
    for k in range(1, 47):  # bucket k holds 2^(k-24) <= |d| < 2^(k-23)
        lo, hi = F32(2.0 ** (k - 24)), F32(2.0 ** (k - 23))
        assert lu.bucket([lo, np.nextafter(hi, F32(0))]).tolist() == [k, k] and lu.bucket([hi])[0] == min(k + 1, 47)
    # inf is a bad row: it reaches no bucket
    w = lu.empty_window()
    Q = np.array([[1, 2, 3], [np.inf, 0, 0], [0, 0, 0]], F32)
    d = lu.fold(w, Q, np.zeros((3, 3), F32), [0, 0, 0], np.zeros(3, F32), np.zeros(3, np.uint8), 0.5)
    assert w["rows"] == 3 and w["rows_bad"] == 1 and w["td_hist"].sum() == 2 and w["act_hist"].tolist()[:3] == [2, 0, 0]
    assert np.isnan(d[1]) and d[0] == 1 and d[2] == 0 and w["td_hist"][24] == 1 and w["td_hist"][0] == 1
    assert w["max_q"] == 3.0 and w["min_q"] == 0.0 and w["max_absd"] == 1.0 and w["s_q"] == 1.0 and w["s_qmax"] == 3.0


def test_first_maximum_ties_and_the_row_arithmetic():
    M = np.array([[1, 3, 3, 2], [5, 5, 5, 5], [-1, -2, -1, -3], [0, np.nan, 7, 7], [np.nan, 9, 9, 9]], F32)
    v, j = lu.first_max(M)
    assert j.tolist() == [1, 0, 0, 2, 0] and v[:4].tolist() == [3, 5, -1, 7] and np.isnan(v[4])
    assert lu.first_min(M)[:3].tolist() == [1, 5, -3]
    Q = np.array([[1, 4, 4], [2, 0, 1], [3, 3, 3]], F32)
    Qt = np.array([[10, 20, 20], [1, 2, 3], [7, 6, 5]], F32)
    r = lu.rows(Q, Qt, act=[1, 7, -3], rew=[1, 2, 3], done=[0, 1, 0], gamma=0.5)
    assert r["a"].tolist() == [1, 2, 0] and r["q"].tolist() == [4, 1, 3] and r["jmax"].tolist() == [1, 0, 0]
    assert r["y"].tolist() == [11, 2, 6.5] and r["d"].tolist() == [-7, -1, -3.5] and not r["bad"].any()
    r = lu.rows(Q, Qt, act=[1, 2, 0], rew=[1, 2, 3], done=[0, 0, 0], gamma=0.5, sel=[-4, 1, 9], gamma_row=[1, 0.25, 2])
    assert r["y"].tolist() == [11, 2.5, 13]
    # greedy counts the raw action against the first maximum; done and the histogram count good rows
    w = lu.empty_window()
    lu.fold(w, Q, Qt, [1, 0, 0], [1, 2, 3], [0, 1, 0], 0.5, loss=2.0, norm=3.0, max_norm=1.0)
    assert (w["n_greedy"], w["n_done"], w["steps"], w["n_clipped"], w["steps_bad"]) == (3, 1, 1, 1, 0)
    assert w["s_loss"] == 2.0 and w["max_norm"] == 3.0
    lu.fold(w, Q, Qt, [2, 1, 1], [1, 2, 3], [0, 1, 0], 0.5, loss=np.nan, norm=0.5, max_norm=1.0)
    assert (w["n_greedy"], w["steps"], w["n_clipped"], w["steps_bad"], w["rows"]) == (3, 2, 1, 1, 6)
    assert w["s_norm"] == 3.0 and w["act_hist"].tolist()[:3] == [2, 3, 1]


def test_block_sum_order():
    # 1 + 2^-53 in block 0 is lost when added to 1.0 first, kept when the small ones meet first
    v = np.zeros(512)
    v[0], v[128], v[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    # tree: s[0] += s[128] (h = 128) loses it; s[1] survives until h = 1: 1.0 + 2^-53 -> 1.0 (ties to even)
    assert lu.block_sum(v) == 1.0
    v[129] = 2.0 ** -53  # s[1] = 2^-52 by h = 128, then s[0] + s[1] = 1 + 2^-52
    assert lu.block_sum(v) == 1.0 + 2.0 ** -52
    big = np.zeros(513)
    big[0], big[256], big[512] = 1e16, 1.0, 1.0  # ascending blocks: (1e16 + 1) + 1 = 1e16, not 1e16 + 2
    assert lu.block_sum(big) == 1e16 and lu.block_sum(big[::-1].copy()) == 1e16 + 2


def test_percentiles_from_a_hand_made_histogram():
    from evacx.lstats import td_percentile
    h = [0] * 48
    h[0], h[24], h[25], h[30] = 10, 40, 40, 10  # 100 rows
    assert td_percentile(h, 0.5, 99.0) == 2.0 ** (24 - 23)   # cumulative 50 reached in bucket 24
    assert td_percentile(h, 0.1, 99.0) == 2.0 ** -23
    assert td_percentile(h, 0.51, 99.0) == 4.0 and td_percentile(h, 0.9, 99.0) == 4.0
    assert td_percentile(h, 0.99, 99.0) == 2.0 ** 7
    h[47] = 100  # 200 rows: the 100th is bucket 30's last, the open-ended bucket reports the maximum
    assert td_percentile(h, 0.99, 1e9) == 1e9 and td_percentile(h, 0.5, 1e9) == 2.0 ** 7
    assert td_percentile(h, 0.45, 1e9) == 4.0
    assert td_percentile([0] * 48, 0.5, None) is None


def test_probe_statistics_from_hand_made_sums():
    from evacx.lstats import probe_stats
    q, g = np.array([1.0, 2.0, 3.0, 4.0]), np.array([2.0, 2.0, 5.0, 7.0])
    e = q - g
    d = probe_stats(4, 1, 2, q.sum(), g.sum(), e.sum(), (e * e).sum(), (q * q).sum(), (g * g).sum(), (q * g).sum(),
                    e.min(), e.max())
    assert (d["probes"], d["bad"], d["open"]) == (4, 1, 2) and d["q0_mean"] == 2.5 and d["return_mean"] == 4.0
    assert d["bias"] == -1.5 and d["rmse"] == math.sqrt(14 / 4) and (d["err_min"], d["err_max"]) == (-3.0, 0.0)
    assert abs(d["corr"] - np.corrcoef(q, g)[0, 1]) < 1e-12
    flat = probe_stats(3, 0, 0, 6.0, 9.0, -3.0, 5.0, 12.0, 29.0, 18.0, -2.0, 0.0)  # q0 always 2: no variance
    assert flat["corr"] is None and flat["bias"] == -1.0
    empty = probe_stats(0, 2, 5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, math.inf, -math.inf)
    assert empty["probes"] == 0 and empty["bad"] == 2 and all(
        empty[k] is None for k in ("q0_mean", "return_mean", "bias", "rmse", "corr", "err_min", "err_max"))


def test_probe_recurrence_and_reduce_order():
    st = lu.probe_state(3)
    Q = np.array([[1, 2], [3, 4], [5, 6], [7, 8], [np.inf, 0], [0, 0]], F32)  # R = 2, A = 2
    act = np.array([1, 0, 5, -1, 0, 0])
    lu.probe_step(st, Q, act, [1.0, 2.0, 3.0], [0, 0, 0], 0.5, 2)
    assert st["q0"].tolist() == [2.5, 6.5, np.inf] and st["open"].tolist() == [1, 1, 1]
    assert st["g"].tolist() == [1, 2, 3]
    lu.probe_step(st, np.zeros_like(Q), act, [4.0, 4.0, 4.0], [1, 0, 1], 0.5, 2)  # open probes keep their q0
    assert st["g"].tolist() == [3, 4, 5] and st["disc"].tolist() == [0.25] * 3 and st["len"].tolist() == [2, 2, 2]
    assert st["open"].tolist() == [0, 1, 0] and st["w_n"].tolist() == [1, 0, 0] and st["w_bad"].tolist() == [0, 0, 1]
    assert st["w_e"][0] == -0.5 and st["w_qg"][0] == 7.5 and st["w_emin"][0] == -0.5 and st["w_emax"][2] == -np.inf
    rows = lu.probe_rows(st, [0, 1, 1], 2)
    assert rows[0][:3] == (1, 0, 0) and rows[1][:3] == (0, 1, 1) and rows[2][:3] == (1, 1, 1) and rows[2][3] == 2.5
    # the strided pass before the tree: env 0 and env 1024 meet first
    v = np.zeros(1025)
    v[0], v[1024], v[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert lu.span_sum(v, np.ones(1025, bool)) == 1.0
    v[0], v[1], v[1024] = 2.0 ** -53, 1.0, 2.0 ** -53
    assert lu.span_sum(v, np.ones(1025, bool)) == 1.0 + 2.0 ** -52
    m = np.ones(1025, bool)
    m[1024] = False
    assert lu.span_sum(v, m) == 1.0


def test_probe_lanes_equal_the_loop():
    rng = np.random.RandomState(5)
    E, R, A = 37, 3, 5
    a, b = lu.probe_state(E), lu.probe_state(E)
    for t in range(30):
        Q = (rng.randn(E * R, A) * 1e4).astype(F32)
        Q[rng.rand(E * R) < 0.03, 2] = np.inf
        act = rng.randint(-1, A + 1, size=E * R)
        rew, done = rng.randn(E) * 300, (rng.rand(E) < 0.15).astype(np.uint8)
        lu.probe_step(a, Q, act, rew, done, 0.99, R)
        half = 20  # two parts of the envs, updated apart
        lu.probe_step_vec(b, Q[:half * R], act[:half * R], rew[:half], done[:half], 0.99, R, 0, half)
        lu.probe_step_vec(b, Q[half * R:], act[half * R:], rew[half:], done[half:], 0.99, R, half, E - half)
        for k in lu.VP_FIELDS:
            f64 = a[k].dtype == np.float64
            assert np.array_equal(lu.bits(a[k]), lu.bits(b[k])) if f64 else np.array_equal(a[k], b[k]), (t, k)
    assert a["w_n"].sum() > 20 and a["w_bad"].sum() > 0
