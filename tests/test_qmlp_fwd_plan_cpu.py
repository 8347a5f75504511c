"""The plan of the MLP forward and act launchers (csrc/qmlp.hip fwd_plan, handed out by
evx_qmlp_fwd_plan_query and evx_qmlp_act_plan_query) pinned on both sides of every edge, and the
argument refusals of the entry points through the queries -- all on a host without a GPU: fake
pointers, nothing launched, no device touched (the act query is given its CU count).

The expected figures restate the rules by hand (blocks = ceil(n / 64), big = ceil(n / 128)):
* fc1: 128-row tiles from big x problems (x nets) >= 384, else 64-row; 256 columns per workgroup with
  128 rows in x3, 512 in bf16, 128 with 64 rows; one x3 problem with fc2 / fc3 outputs: 64 x 256 always;
* fc23: 64 rows; single-net x3: 32 rows while blocks x problems < 256;
* evx_qmlp_forward2 in x3 with a target that wants Q only: both nets through their act tables in one
  launch for 8192 <= n < 32768 (tables on both nets, every output of the online net, one dropout
  mode); from 32768 the target through the fused act kernel and the online net through its table, or
  without one through qfc1 + qfc23 alone; otherwise the two-problem qfc1 + qfc23;
* x3 act: the persistent kernel from big >= 4 x CUs with a table, without an explicit mask and
  without kernel64 -- min(big, CUs) workgroups, the rest on min(2 big, CUs) with a workspace and
  ceil(n / 1024) without; else the 64-row kernel.
Not reached from here: evx_qmlp_stat and evx_qmlp_stat_x have no query (the two queries take the
forward's and the act's arguments). evx_qmlp_stat's tile is pinned through the launch it is -- one
forward with no fc2 / fc3 output, the `fc1-only` cases: the same branch of the plan -- and
evx_qmlp_stat_x's fixed 64 x 128 tile, like the raw-table record both build, runs only in the GPU
tests of the act table (tests/test_qmlp_x3_gpu.py, tests/test_target_table_gpu.py).
The GPU tests that exist to run one of these routes assert it through the same queries, so a re-tuned
threshold fails here (the pin) and there (the case's route)."""
import ctypes
import os
import re

import pytest

from golden_util import ROOT
from test_qgroup_plan_cpu import PINS as GROUP_PINS

FAKE = 0x1000  # a non-null address that is never dereferenced
L_, W_ = 36, 30


def _lib():
    from evacx import _lib
    return _lib


def _lay(**kw):
    f = dict(L=L_, W=W_, danger_o32=FAKE, cellinfo=FAKE, obs_feat=FAKE, obs_feat_lo=FAKE)
    f.update(kw)
    return _lib().evx_layout(**f)


def _par(x3=True, table=False, **kw):
    f = dict(w1=FAKE, b1c=FAKE, w2=FAKE, b2=FAKE, w3=FAKE, b3=FAKE)
    if x3:
        f.update(x3=1, w1l=FAKE, w2l=FAKE)
    if table:
        f.update(w1o=FAKE, stat=FAKE, stat_fs=7)
        if x3:
            f.update(w1ol=FAKE)
    f.update(kw)
    return _lib().evx_qmlp_params(**f)


def _drop(mode=1, **kw):
    """mode 0: off, 1: the hash, 2: an explicit mask"""
    f = dict(seed=1, stream=2, p=0.2 if mode else 0.0)
    if mode == 2:
        f.update(mask=FAKE)
    f.update(kw)
    return _lib().evx_qmlp_dropout(**f)


def _out(names, **kw):
    return _lib().evx_qmlp_fwd_out(**{k: FAKE for k in names.split()}, **kw)


ONLINE, TARGET = "h1 x h2 q", "h1 q"  # the learner's outputs: everything the backward reads / Q only


def _ref(x):
    return None if x is None else ctypes.byref(x) if isinstance(x, ctypes.Structure) else x


def fwd_query(n, p0, out0, p1=None, out1=None, drop0=None, drop1=None, nets=0, lay=None, plan=True):
    """(rc, plan, text) of evx_qmlp_fwd_plan_query; p1 = out1 = None: the single forward"""
    m = _lib()
    lay = _lay() if lay is None else lay
    pl = m.evx_qmlp_fwd_plan(*[7] * 10)
    one = p1 is None and out1 is None
    rc = m.lib().evx_qmlp_fwd_plan_query(_ref(lay), n, FAKE, _ref(p0), _ref(drop0), _ref(out0), None if one else FAKE,
                                         _ref(p1), _ref(drop1), _ref(out1), nets, _ref(pl) if plan else None)
    return rc, pl, m.lib().evx_qmlp_last_error()


def act_query(n, p, out, drop=None, nets=0, kernel64=False, ncu=256, lay=None, plan=True):
    m = _lib()
    lay = _lay() if lay is None else lay
    pl = m.evx_qmlp_fwd_plan(*[7] * 10)
    rc = m.lib().evx_qmlp_act_plan_query(_ref(lay), FAKE, n, _ref(p), _ref(drop), _ref(out), nets, int(kernel64), ncu,
                                         _ref(pl) if plan else None)
    return rc, pl, m.lib().evx_qmlp_last_error()


def _fields(pl):
    return {n: getattr(pl, n) for n, _ in pl._fields_}


def _pair(n, table=False, x3=True, dm0=1, dm1=1, out0=ONLINE, out1=TARGET, table1=None):
    return fwd_query(n, _par(x3, table), _out(out0), _par(x3, table if table1 is None else table1), _out(out1),
                     _drop(dm0), _drop(dm1))


def _single(n, outs, x3=True):
    return fwd_query(n, _par(x3), _out(outs), drop0=_drop(1))


def _act(n, table=True, x3=True, dm=1, ws=False, **kw):
    return act_query(n, _par(x3, table), _out("q actions", **({"act_ws": FAKE} if ws else {})), _drop(dm), **kw)


def _fc(rows, cols, fc23, **kw):
    return dict(route="FC", fc1_rows=rows, fc1_cols=cols, fc23_rows=fc23, **kw)


# name -> (query, the fields it pins; every field not named is 0, drop_mode / drop_mode1 are 1)
PLAN_PINS = {
    # evx_qmlp_forward2, x3, act tables on both nets, the target wants Q only
    "pair-table-8191": (lambda: _pair(8191, True), _fc(64, 128, 64)),
    "pair-table-8192": (lambda: _pair(8192, True), dict(route="PAIRED", x_expand=1)),
    "pair-table-32767": (lambda: _pair(32767, True), dict(route="PAIRED", x_expand=1)),
    "pair-table-32768": (lambda: _pair(32768, True), dict(route="TARGET_ACT_TABLE", x_expand=1)),
    "pair-table-8192-hash-and-mask": (lambda: _pair(8192, True, dm0=1, dm1=2), _fc(64, 128, 64, drop_mode1=2)),
    "pair-table-8192-masks": (lambda: _pair(8192, True, dm0=2, dm1=2),
                              dict(route="PAIRED", x_expand=1, drop_mode=2, drop_mode1=2)),
    "pair-table-8192-no-dropout": (lambda: _pair(8192, True, dm0=0, dm1=0),
                                   dict(route="PAIRED", x_expand=1, drop_mode=0, drop_mode1=0)),
    # ... the paired form needs the target's table, every output of the online net and a Q-only target
    "pair-online-table-only-8192": (lambda: _pair(8192, True, table1=False), _fc(64, 128, 64)),
    "pair-table-8192-no-x": (lambda: _pair(8192, True, out0="h1 h2 q"), _fc(64, 128, 64)),
    "pair-table-8192-target-h2": (lambda: _pair(8192, True, out1="h1 h2 q"), _fc(64, 128, 64)),
    # ... from 32768 the target's act needs no table; the online net without x saved keeps qfc1 + qfc23
    "pair-online-table-only-32768": (lambda: _pair(32768, True, table1=False),
                                     dict(route="TARGET_ACT_TABLE", x_expand=1)),
    "pair-table-32768-no-x": (lambda: _pair(32768, True, out0="h1 h2 q"),
                              dict(route="TARGET_ACT_FC", fc1_rows=64, fc1_cols=256, fc23_rows=64)),
    "pair-table-32768-target-h2": (lambda: _pair(32768, True, out1="h1 h2 q"), _fc(128, 256, 64)),
    # the same without tables
    "pair-32767": (lambda: _pair(32767), _fc(128, 256, 64)),
    "pair-32768": (lambda: _pair(32768), dict(route="TARGET_ACT_FC", fc1_rows=64, fc1_cols=256, fc23_rows=64)),
    "pair-32768-hash-and-mask": (lambda: _pair(32768, dm0=2, dm1=1),
                                 dict(route="TARGET_ACT_FC", fc1_rows=64, fc1_cols=256, fc23_rows=64, drop_mode=2)),
    "pair-24448": (lambda: _pair(24448), _fc(64, 128, 64)),    # 191 x 2 tiles
    "pair-24449": (lambda: _pair(24449), _fc(128, 256, 64)),   # 192 x 2
    "pair-8128": (lambda: _pair(8128), _fc(64, 128, 32)),      # 127 x 2 blocks
    "pair-8129": (lambda: _pair(8129), _fc(64, 128, 64)),      # 128 x 2
    "pair-1": (lambda: _pair(1), _fc(64, 128, 32)),
    # the single x3 forward with fc2 / fc3 outputs: 64 x 256 at any n
    "single-16320": (lambda: _single(16320, "h1 q"), _fc(64, 256, 32)),   # 255 blocks
    "single-16321": (lambda: _single(16321, "h1 q"), _fc(64, 256, 64)),   # 256
    "single-49025-h2": (lambda: _single(49025, "h1 h2"), _fc(64, 256, 64)),
    # fc1 alone (evx_qmlp_stat's launch: the same rule, no fc2 / fc3 output)
    "fc1-only-49024": (lambda: _single(49024, "h1"), _fc(64, 128, 0)),    # 383 tiles
    "fc1-only-49025": (lambda: _single(49025, "h1"), _fc(128, 256, 0)),   # 384
    # bf16
    "bf16-pair-24448": (lambda: _pair(24448, x3=False), _fc(64, 128, 64)),
    "bf16-pair-24449": (lambda: _pair(24449, x3=False), _fc(128, 512, 64)),
    "bf16-pair-table-32768": (lambda: _pair(32768, True, x3=False), _fc(128, 512, 64)),  # the act forms are x3's
    "bf16-single-49024": (lambda: _single(49024, "h1 q", x3=False), _fc(64, 128, 64)),
    "bf16-single-49025": (lambda: _single(49025, "h1 q", x3=False), _fc(128, 512, 64)),
    # nothing to do
    "pair-0": (lambda: _pair(0, True), dict(route="NONE", drop_mode=0, drop_mode1=0)),
    "act-0": (lambda: _act(0), dict(route="NONE", drop_mode=0, drop_mode1=0)),
    # the x3 act with a table on 256 CUs
    "act-130944": (lambda: _act(130944), dict(route="ACT_64")),            # 1023 tiles
    "act-130945": (lambda: _act(130945), dict(route="ACT_PERSISTENT", act_grid=256, rest_grid=128)),  # 1024
    "act-130945-ws": (lambda: _act(130945, ws=True),
                      dict(route="ACT_PERSISTENT", act_grid=256, rest_grid=256, rest_listed=1)),
    "act-130945-no-dropout": (lambda: _act(130945, dm=0),
                              dict(route="ACT_PERSISTENT", act_grid=256, rest_grid=128, drop_mode=0, drop_mode1=0)),
    "act-130945-kernel64": (lambda: _act(130945, kernel64=True), dict(route="ACT_64")),
    "act-130945-mask": (lambda: _act(130945, dm=2), dict(route="ACT_64", drop_mode=2, drop_mode1=2)),
    "act-130945-no-table": (lambda: _act(130945, table=False), dict(route="ACT_64")),
    "act-130945-304-cus": (lambda: _act(130945, ncu=304), dict(route="ACT_64")),
    "act-155648-304-cus": (lambda: _act(155648, ncu=304, ws=True),    # 1216 tiles = 4 x 304
                           dict(route="ACT_PERSISTENT", act_grid=304, rest_grid=304, rest_listed=1)),
    "act-1024-8-cus": (lambda: _act(4096, ncu=8), dict(route="ACT_PERSISTENT", act_grid=8, rest_grid=4)),
    # the bf16 act and the grouped act
    "act-bf16": (lambda: _act(130945, x3=False), dict(route="ACT_BF16")),
    "act-grouped": (lambda: act_query(62, _par(), _out("q"), _drop(1), nets=16), dict(route="ACT_GROUPED")),
    "act-grouped-1-net": (lambda: act_query(62, _par(), _out("actions"), _drop(2), nets=1),
                          dict(route="ACT_GROUPED", drop_mode=2, drop_mode1=2)),
}


@pytest.mark.parametrize("name", sorted(PLAN_PINS))
def test_plan_at_the_edges(name):
    query, pins = PLAN_PINS[name]
    rc, pl, text = query()
    assert rc == 0, text
    want = dict(route=0, fc1_rows=0, fc1_cols=0, fc23_rows=0, drop_mode=1, drop_mode1=1, x_expand=0, act_grid=0,
                rest_grid=0, rest_listed=0)
    want.update(pins)
    want["route"] = _lib().FWD[want["route"]]
    assert _fields(pl) == want


@pytest.mark.parametrize("nets,B", sorted(GROUP_PINS), ids=[f"{g}x{b}" for g, b in sorted(GROUP_PINS)])
def test_grouped_forward_takes_the_group_plans_fc1_tile(nets, B):
    """evx_qmlp_forward2_g at every key of tests/test_qgroup_plan_cpu.py's PINS: fc1's rows are
    evx_qmlp_group_plan's; one net runs the single-net instantiations (with their 32-row fc23 rule)."""
    from evacx.qgroup import group_plan
    rc, pl, text = fwd_query(B, _par(), _out(ONLINE), _par(), _out(TARGET), _drop(1), _drop(1), nets=nets)
    assert rc == 0, text
    rows = group_plan(B, nets).fc1_rows
    assert rows == GROUP_PINS[(nets, B)][0]
    want = dict(route="FC_GROUPED" if nets > 1 else "FC", fc1_rows=rows, fc1_cols=256 if rows == 128 else 128,
                fc23_rows=32 if nets == 1 and -(-B // 64) * 2 < 256 else 64)
    got = _fields(pl)
    assert {k: got[k] for k in want} == dict(want, route=_lib().FWD[want["route"]])


def test_every_route_constant_is_pinned():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evacx.h")).read(), flags=re.S)
    routes = re.findall(r"#define EVX_FWD_(\w+)", header)
    assert len(routes) == len(set(routes)) == len(_lib().FWD) >= 10
    pinned = {pins["route"] for _, pins in PLAN_PINS.values()} | {"FC_GROUPED"}  # (the grouped forward's test)
    assert sorted(pinned) == sorted(routes)


def _restated_pair_route(n, tables):
    if n >= 32768:
        return "TARGET_ACT_TABLE" if tables else "TARGET_ACT_FC"
    return "PAIRED" if tables and n >= 8192 else "FC"


def test_pair_plan_follows_the_restated_rules_around_every_edge():
    """The learner's x3 pair (tables on both nets or on neither) at every n around the edges, against
    the module docstring's rules written out in Python."""
    FWD = _lib().FWD
    edges = (1, 8128, 8192, 24448, 32768, 49024)
    for tables in (False, True):
        for n in sorted({e + d for e in edges for d in range(-130, 131) if e + d > 0}):
            rc, pl, text = _pair(n, tables)
            assert rc == 0, text
            route = _restated_pair_route(n, tables)
            blocks, big = -(-n // 64), -(-n // 128)
            if route == "FC":
                rows = 128 if big * 2 >= 384 else 64
                want = (rows, 256 if rows == 128 else 128, 32 if blocks * 2 < 256 else 64, 0)
            elif route == "TARGET_ACT_FC":
                want = (64, 256, 64, 0)
            else:
                want = (0, 0, 0, 1)
            assert (pl.route, pl.fc1_rows, pl.fc1_cols, pl.fc23_rows, pl.x_expand) == (FWD[route],) + want, (n, tables)


def test_act_plan_follows_the_restated_rules_around_the_edge():
    FWD = _lib().FWD
    for ncu in (8, 256, 304):
        for ws in (False, True):
            for n in range(128 * 4 * ncu - 300, 128 * 4 * ncu + 300, 7):
                rc, pl, text = _act(n, ncu=ncu, ws=ws)
                assert rc == 0, text
                big = -(-n // 128)
                if big >= 4 * ncu:
                    want = (FWD["ACT_PERSISTENT"], min(big, ncu), min(2 * big, ncu) if ws else -(-n // 1024), int(ws))
                else:
                    want = (FWD["ACT_64"], 0, 0, 0)
                assert (pl.route, pl.act_grid, pl.rest_grid, pl.rest_listed) == want, (n, ncu, ws)


# ------------------------------------------------------------------------------------- refusals
def _launch_pair(n, p0, out0, p1, out1, drop0=None, drop1=None, nets=0, lay=None):
    """The launch with the arguments of fwd_query (every case here is refused before any device call)."""
    L = _lib().lib()
    lay = _lay() if lay is None else lay
    if p1 is None and out1 is None:
        return L.evx_qmlp_forward(_ref(lay), FAKE, n, _ref(p0), _ref(drop0), _ref(out0), None)
    if nets:
        return L.evx_qmlp_forward2_g(_ref(lay), n, nets, FAKE, _ref(p0), _ref(drop0), _ref(out0), FAKE, _ref(p1),
                                     _ref(drop1), _ref(out1), None)
    return L.evx_qmlp_forward2(_ref(lay), n, FAKE, _ref(p0), _ref(drop0), _ref(out0), FAKE, _ref(p1), _ref(drop1),
                               _ref(out1), None)


def _fwd_refusals():
    m = _lib()
    x3, on, tg = _par(), _out(ONLINE), _out(TARGET)
    single = lambda **kw: dict(dict(n=64, p0=x3, out0=on), **kw)  # noqa: E731
    pair = lambda **kw: dict(dict(n=64, p0=x3, out0=on, p1=x3, out1=tg), **kw)  # noqa: E731
    return {
        # make_fwd's, on the first and on the second problem
        "null-params": (single(p0=None), b"qmlp_forward: NULL argument"),
        "null-out": (single(out0=None), b"qmlp_forward: NULL argument"),
        "null-second-out": (pair(out1=None), b"qmlp_forward: NULL argument"),
        "missing-parameter": (single(p0=_par(w3=None)), b"qmlp_forward: missing parameter"),
        "missing-parameter-second": (pair(p1=_par(b1c=None)), b"qmlp_forward: missing parameter"),
        "no-h1": (single(out0=_out("q")), b"qmlp_forward: h1 buffer required"),
        "no-h1-second": (pair(out1=_out("q")), b"qmlp_forward: h1 buffer required"),
        "layout-tables": (single(lay=_lay(obs_feat=None)), b"qmlp_forward: layout tables missing (obs_feat)"),
        "odd-row0": (single(drop0=_drop(1, row0=3)), b"qmlp_forward: dropout row0 must be even (one hash per row pair)"),
        "table-range": (single(p0=_par(table=True, stat_x0=5, stat_nx=L_ + 2)),
                        b"qmlp: the table's centre range must lie in [0, L + 2)"),
        "mask-without-p": (single(drop0=m.evx_qmlp_dropout(mask=FAKE)),
                           b"qmlp_forward: an explicit dropout mask needs p > 0 (its scale)"),
        "x3-lo-weights": (single(p0=_par(w1l=None)), b"qmlp_forward: x3 needs w1l / w2l (evx_qmlp_pack3)"),
        "x3-lo-features": (single(lay=_lay(obs_feat_lo=None)), b"qmlp_forward: x3 needs the layout's obs_feat_lo"),
        "odd-rows-per-env": (single(out0=_out(ONLINE + " perm", rows_per_env=3)),
                             b"qmlp_forward: rows_per_env must be even (dropout row pairs)"),
        # evx_qmlp_forward2's
        "pair-needs-fc23": (pair(out1=_out("h1")), b"qmlp_forward2: both problems need an fc2/fc3 output"),
        "pair-one-precision": (pair(p1=_par(x3=False)), b"qmlp_forward2: both problems in one precision"),
        # evx_qmlp_forward2_g's
        "group-nets-low": (pair(nets=-1), b"grouped qmlp: nets must be 1..1024"),
        "group-nets-high": (pair(nets=1025), b"grouped qmlp: nets must be 1..1024"),
        "group-x3": (pair(nets=2, p1=_par(x3=False)),
                     b"grouped qmlp: x3 parameters required (the [nets] operand layout is x3's)"),
        "group-odd-rows": (pair(nets=2, n=63), b"qmlp_forward2_g: rows per net must be even (dropout row pairs)"),
        "group-table": (pair(nets=2, p0=_par(table=True)), b"qmlp_forward2_g: no table path / permutation"),
        "group-perm": (pair(nets=2, out1=_out(TARGET + " perm", rows_per_env=2)),
                       b"qmlp_forward2_g: no table path / permutation"),
        "group-needs-fc23": (pair(nets=2, out1=_out("h1 actions")), b"qmlp_forward2_g: needs fc2/fc3 outputs"),
        "group-too-many-rows": (pair(nets=1024, n=1 << 21), b"qmlp_forward2_g: too many rows"),
    }


@pytest.mark.parametrize("name", sorted(_fwd_refusals()))
def test_forward_query_refuses_as_the_launch_does(name):
    kw, text = _fwd_refusals()[name]
    L = _lib().lib()
    assert _launch_pair(kw["n"], kw["p0"], kw["out0"], kw.get("p1"), kw.get("out1"), kw.get("drop0"), kw.get("drop1"),
                        kw.get("nets", 0), kw.get("lay")) == -22
    assert L.evx_qmlp_last_error() == text
    # another text in between, so that the query's is its own
    assert L.evx_qmlp_pack(*[None] * 9) == -22 and L.evx_qmlp_last_error() != text
    rc, pl, got = fwd_query(**kw)
    assert rc == -22 and got == text
    assert set(_fields(pl).values()) == {0}  # a refused query leaves no stale figures


def _act_refusals():
    x3, q = _par(), _out("q")
    return {
        "null-out": (dict(n=64, p=x3, out=None), b"qmlp_act: NULL out"),
        "no-output": (dict(n=64, p=x3, out=_out("")), b"qmlp_act: needs q or actions"),
        "null-params": (dict(n=64, p=None, out=q), b"qmlp_forward: NULL argument"),
        "x3-lo-weights": (dict(n=64, p=_par(w2l=None), out=q), b"qmlp_forward: x3 needs w1l / w2l (evx_qmlp_pack3)"),
        "odd-rows-per-env": (dict(n=64, p=x3, out=_out("q perm", rows_per_env=1)),
                             b"qmlp_forward: rows_per_env must be even (dropout row pairs)"),
        "group-nets": (dict(n=62, p=x3, out=q, nets=1025), b"grouped qmlp: nets must be 1..1024"),
        "group-x3": (dict(n=62, p=_par(x3=False), out=q, nets=16),
                     b"grouped qmlp: x3 parameters required (the [nets] operand layout is x3's)"),
        "group-no-output": (dict(n=62, p=x3, out=None, nets=16), b"qmlp_act_g: needs q or actions"),
        "group-perm": (dict(n=62, p=x3, out=_out("q perm"), nets=16), b"qmlp_act_g: no act permutation with grouped nets"),
        "group-table": (dict(n=62, p=_par(table=True), out=q, nets=16), b"qmlp_act_g: the act table path is single-net"),
        "group-odd-rows": (dict(n=63, p=x3, out=q, nets=16), b"qmlp_act_g: rows per net must be even (dropout row pairs)"),
    }


@pytest.mark.parametrize("name", sorted(_act_refusals()))
def test_act_query_refuses_as_the_launch_does(name):
    kw, text = _act_refusals()[name]
    L = _lib().lib()
    lay, nets = _lay(), kw.get("nets", 0)
    if nets:
        rc = L.evx_qmlp_act_g(_ref(lay), FAKE, kw["n"], nets, _ref(kw["p"]), None, _ref(kw["out"]), None)
    else:
        rc = L.evx_qmlp_act(_ref(lay), FAKE, kw["n"], _ref(kw["p"]), None, _ref(kw["out"]), None)
    assert rc == -22 and L.evx_qmlp_last_error() == text
    assert L.evx_qmlp_pack(*[None] * 9) == -22 and L.evx_qmlp_last_error() != text
    rc, pl, got = act_query(**kw)
    assert rc == -22 and got == text
    assert set(_fields(pl).values()) == {0}


def test_queries_refuse_a_null_plan():
    rc, _, text = fwd_query(64, _par(), _out(ONLINE), plan=False)
    assert rc == -22 and text == b"qmlp_fwd_plan_query: NULL plan"
    rc, _, text = act_query(64, _par(), _out("q"), plan=False)
    assert rc == -22 and text == b"qmlp_act_plan_query: NULL plan"


def test_stat_entry_points_keep_their_refusals():
    """evx_qmlp_stat and evx_qmlp_stat_x share one body; each keeps its own texts (x = NULL: evx_qmlp_stat)."""
    L = _lib().lib()
    lay, x3 = _lay(), _par()
    for call, text in (
            (lambda: L.evx_qmlp_stat(_ref(lay), FAKE, 64, _ref(x3), None, None), b"qmlp_stat: NULL out"),
            (lambda: L.evx_qmlp_stat_x(_ref(lay), FAKE, None, 64, _ref(x3), None, None), b"qmlp_stat: NULL out"),
            (lambda: L.evx_qmlp_stat(_ref(lay), FAKE, 64, None, FAKE, None), b"qmlp_forward: NULL argument"),
            (lambda: L.evx_qmlp_stat_x(_ref(lay), FAKE, FAKE, 64, None, FAKE, None), b"qmlp_stat_x: NULL argument"),
            (lambda: L.evx_qmlp_stat_x(_ref(lay), FAKE, FAKE, 64, _ref(x3), None, None), b"qmlp_stat_x: NULL argument"),
            (lambda: L.evx_qmlp_stat_x(_ref(lay), FAKE, FAKE, 64, _ref(_par(x3=False)), FAKE, None),
             b"qmlp_stat_x: the X input is the x3 layout (p->x3)"),
            (lambda: L.evx_qmlp_stat(_ref(lay), FAKE, 64, _ref(_par(table=True, stat_x0=5, stat_nx=L_ + 2)), FAKE, None),
             b"qmlp: the table's centre range must lie in [0, L + 2)")):
        assert call() == -22
        assert L.evx_qmlp_last_error() == text
    assert L.evx_qmlp_stat(None, None, 0, None, None, None) == 0  # no rows: nothing to do
    assert L.evx_qmlp_stat_x(None, None, FAKE, 0, None, None, None) == 0
