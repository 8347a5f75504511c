"""Population training without a GPU: every -22 refusal of the four device entries with its message
(fake pointers, nothing launched), the plan query's route for evx_qmlp_act_gb, PopulationTrainer's
constructor refusals that need no device, and the runner's argument broadcasting."""
import ctypes
import os
import sys
import types

import pytest

from golden_util import ROOT

FAKE = 0x1000  # a non-null address that is never dereferenced


def _m():
    from evacx import _lib
    return _lib


def _lay():
    return _m().evx_layout(L=36, W=30, danger_o32=FAKE, cellinfo=FAKE, obs_feat=FAKE, obs_feat_lo=FAKE)


def _par(**kw):
    f = dict(w1=FAKE, b1c=FAKE, w2=FAKE, b2=FAKE, w3=FAKE, b3=FAKE, x3=1, w1l=FAKE, w2l=FAKE)
    f.update(kw)
    return _m().evx_qmlp_params(**f)


def _eps(*v):
    return (ctypes.c_float * len(v))(*v)


def _act_query(n=62, nets=3, par=None, out=None, eps=None, obs=FAKE, lay=True, drop=True, plan=True, launch=False):
    """(rc, plan, text) of evx_qmlp_act_gb_plan_query -- or of evx_qmlp_act_gb itself (launch).
    par / out / eps: None for a valid default, False for a NULL pointer."""
    m = _m()
    par = _par() if par is None else par
    out = m.evx_qmlp_fwd_out(q=FAKE, actions=FAKE) if out is None else out
    eps = _eps(*[0.1] * max(nets, 1)) if eps is None else eps
    d = m.evx_qmlp_dropout(seed=1, stream=2, p=0.2)
    pl = m.evx_qmlp_fwd_plan(*[7] * 10)
    args = (ctypes.byref(_lay()) if lay else None, obs, n, nets, None if par is False else ctypes.byref(par),
            ctypes.byref(d) if drop else None, None if out is False else ctypes.byref(out),
            None if eps is False else eps)
    if launch:
        rc = m.lib().evx_qmlp_act_gb(*args, None)
    else:
        rc = m.lib().evx_qmlp_act_gb_plan_query(*args, ctypes.byref(pl) if plan else None)
    return rc, pl, m.lib().evx_last_error().decode()


def test_act_gb_plan_is_the_new_route():
    m = _m()
    assert m.FWD_ACT_GROUPED_BLOCKED == 10 and m.FWD_ACT_GROUPED_BLOCKED not in m.FWD.values()
    header = open(os.path.join(ROOT, "include", "evacx.h")).read()
    assert "EVX_FWD_ACT_GROUPED_BLOCKED = 10" in header
    for n, nets, dm in ((2, 1, 1), (62, 3, 1), (128, 64, 0), (4096, 8, 2)):
        d = dict(p=0.0) if dm == 0 else dict(mask=FAKE) if dm == 2 else {}
        drop = m.evx_qmlp_dropout(seed=1, stream=2, **dict(dict(p=0.2), **d))
        pl = m.evx_qmlp_fwd_plan(*[7] * 10)
        out, par = m.evx_qmlp_fwd_out(actions=FAKE), _par()
        rc = m.lib().evx_qmlp_act_gb_plan_query(ctypes.byref(_lay()), FAKE, n, nets, ctypes.byref(par),
                                                ctypes.byref(drop), ctypes.byref(out), _eps(*[0.5] * nets),
                                                ctypes.byref(pl))
        assert rc == 0, m.lib().evx_last_error()
        got = {k: getattr(pl, k) for k, _ in pl._fields_}
        want = dict.fromkeys(got, 0)
        want.update(route=m.FWD_ACT_GROUPED_BLOCKED, drop_mode=dm, drop_mode1=dm)
        assert got == want, (n, nets)
    rc, pl, _ = _act_query(n=0)
    assert rc == 0 and pl.route == m.FWD["NONE"]


# name -> (the query's arguments, made when the test runs; the text)
ACT_REFUSALS = {
    "no-plan": (lambda: dict(plan=False), "qmlp_act_gb_plan_query: NULL plan"),
    "no-epsilon": (lambda: dict(eps=False), "qmlp_act_gb: NULL argument"),
    "no-obs": (lambda: dict(obs=None), "qmlp_act_gb: NULL argument"),
    "no-layout": (lambda: dict(lay=False), "qmlp_act_gb: NULL argument"),
    "no-params": (lambda: dict(par=False), "qmlp_act_gb: NULL argument"),
    "no-out": (lambda: dict(out=False), "qmlp_act_gb: NULL argument"),
    "nets-0": (lambda: dict(nets=0), "qmlp_act_gb: nets must be 1..64"),
    "nets-65": (lambda: dict(nets=65, eps=_eps(*[0.0] * 65)), "qmlp_act_gb: nets must be 1..64"),
    "odd-n": (lambda: dict(n=63), "qmlp_act_gb: rows per net must be even (dropout row pairs)"),
    "nan-epsilon": (lambda: dict(eps=_eps(0.1, float("nan"), 0.1)), "qmlp_act_gb: epsilon must be finite"),
    "inf-epsilon": (lambda: dict(eps=_eps(0.1, 0.1, float("inf"))), "qmlp_act_gb: epsilon must be finite"),
    "bf16-params": (lambda: dict(par=_par(x3=0)),
                    "grouped qmlp: x3 parameters required (the [nets] operand layout is x3's)"),
    "act-table": (lambda: dict(par=_par(stat=FAKE, w1o=FAKE, w1ol=FAKE)),
                  "qmlp_act_gb: the act table path is single-net"),
    "no-output": (lambda: dict(out=_m().evx_qmlp_fwd_out()), "qmlp_act_gb: needs q or actions"),
    "permutation": (lambda: dict(out=_m().evx_qmlp_fwd_out(q=FAKE, perm=FAKE, rows_per_env=4)),
                    "qmlp_act_gb: no act permutation with grouped nets"),
    "act-ws": (lambda: dict(out=_m().evx_qmlp_fwd_out(q=FAKE, act_ws=FAKE)),
               "qmlp_act_gb: no act workspace with grouped nets"),
}


@pytest.mark.parametrize("name", sorted(ACT_REFUSALS))
def test_act_gb_refusals(name):
    """The query and (where the query is not what is refused) the launcher itself return -22 with the
    same text, before any launch: the host has no device."""
    make, text = ACT_REFUSALS[name]
    kw = make()
    rc, _, got = _act_query(**kw)
    assert (rc, got) == (-22, text)
    if name != "no-plan":
        rc, _, got = _act_query(launch=True, **kw)
        assert (rc, got) == (-22, text)


def _adam(nets=3, lr=(1e-3, 1e-3, 1e-3), h=True, null=None):
    m = _m()
    hyper = m.evx_adam(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1)
    ptrs = [FAKE] * 4 + [1.0, ctypes.byref(hyper) if h else None] + [FAKE] * 10 + [4, FAKE, nets]
    if null is not None:
        ptrs[null] = None
    lrs = None if lr is None else (ctypes.c_float * len(lr))(*lr)
    rc = m.lib().evx_qmlp_adam_pack3_gl(*ptrs, lrs, None)
    return rc, m.lib().evx_last_error().decode()


def test_adam_pack3_gl_refusals():
    assert _adam(lr=None) == (-22, "qmlp_adam_pack3_gl: NULL lr")
    assert _adam(nets=0) == (-22, "qmlp_adam_pack3_gl: nets must be 1..64")
    assert _adam(nets=65, lr=[1e-3] * 65) == (-22, "qmlp_adam_pack3_gl: nets must be 1..64")
    assert _adam(lr=(1e-3, float("nan"), 1e-3)) == (-22, "qmlp_adam_pack3_gl: lr must be finite")
    assert _adam(lr=(float("-inf"), 1e-3, 1e-3)) == (-22, "qmlp_adam_pack3_gl: lr must be finite")
    assert _adam(h=False) == (-22, "qmlp_adam_pack3: NULL argument")
    for i in (0, 1, 2, 3, 6, 7, 8, 9, 10, 15):  # p, g, m, v, w1b, w1l, b1c, w2b, w2l, ss
        assert _adam(null=i) == (-22, "qmlp_adam_pack3: NULL argument"), i
    assert _adam(null=13) == (-22, "qmlp_adam_pack3: w1o and w1ol go together")


def _ring(cap=512, **kw):
    f = dict(capacity=cap, s=FAKE, s2=FAKE, a=FAKE, r=FAKE, done=FAKE)
    f.update(kw)
    return _m().evx_replay(**f)


def _push(rp=True, n=128, nets=3, apn=4, pos=0, null=None, ring=None):
    m = _m()
    ring = _ring() if ring is None else ring
    ptrs = [FAKE] * 6  # s, s2, s2_term, a, r_env, done_env
    if null is not None:
        ptrs[null] = None
    rc = m.lib().evx_replay_push_blocks(ctypes.byref(ring) if rp else None, *ptrs, n, nets, apn, pos, None)
    return rc, m.lib().evx_last_error().decode()


def test_replay_push_blocks_refusals():
    assert _push(rp=False) == (-22, "replay_push_blocks: NULL argument")
    for i in (0, 1, 3, 4, 5):  # (s2_term, index 2, may be NULL)
        assert _push(null=i) == (-22, "replay_push_blocks: NULL argument"), i
    assert _push(ring=_ring(s2=None)) == (-22, "replay_push_blocks: NULL ring array")
    assert _push(nets=0) == (-22, "replay_push_blocks: nets must be 1..64")
    assert _push(nets=65) == (-22, "replay_push_blocks: nets must be 1..64")
    assert _push(n=127) == (-22, "replay_push_blocks: rows per ring must be even and >= 0")
    assert _push(n=-2) == (-22, "replay_push_blocks: rows per ring must be even and >= 0")
    assert _push(n=514) == (-22, "replay_push_blocks: the capacity does not hold n rows")
    assert _push(ring=_ring(cap=0), n=0) == (-22, "replay_push_blocks: the capacity does not hold n rows")
    assert _push(n=126) == (-22, "replay_push_blocks: rows per ring must be a multiple of agents_per_env")
    assert _push(apn=0) == (-22, "replay_push_blocks: rows per ring must be a multiple of agents_per_env")
    assert _push(pos=512) == (-22, "replay_push_blocks: pos outside [0, capacity)")
    assert _push(pos=-1) == (-22, "replay_push_blocks: pos outside [0, capacity)")
    assert _push(n=0)[0] == 0  # nothing to push: nothing launched


def _sample(rp=True, size=512, B=256, nets=3, null=None, ring=None):
    m = _m()
    ring = _ring() if ring is None else ring
    ptrs = [FAKE] * 5
    if null is not None:
        ptrs[null] = None
    rc = m.lib().evx_replay_sample_blocks(ctypes.byref(ring) if rp else None, size, B, nets, 18, 0, *ptrs, None)
    return rc, m.lib().evx_last_error().decode()


def test_replay_sample_blocks_refusals():
    assert _sample(rp=False) == (-22, "replay_sample_blocks: NULL argument")
    for i in range(5):
        assert _sample(null=i) == (-22, "replay_sample_blocks: NULL argument"), i
    assert _sample(ring=_ring(done=None)) == (-22, "replay_sample_blocks: NULL ring array")
    assert _sample(nets=0) == (-22, "replay_sample_blocks: nets must be 1..64")
    assert _sample(nets=65) == (-22, "replay_sample_blocks: nets must be 1..64")
    assert _sample(B=255) == (-22, "replay_sample_blocks: B must be even and >= 0")
    assert _sample(size=0) == (-22, "replay_sample_blocks: size outside [1, capacity]")
    assert _sample(size=513) == (-22, "replay_sample_blocks: size outside [1, capacity]")
    assert _sample(size=200) == (-22, "replay_sample_blocks: sample larger than a ring's population (random.sample)")
    assert _sample(B=0)[0] == 0  # nothing to draw: nothing launched


def test_population_trainer_refusals_need_no_device():
    from evacx.env import LayoutSet
    from evacx.population import PopulationTrainer
    lay = types.SimpleNamespace(R=4, P=300, device="cpu")
    ok = dict(members=3, batch=256, replay_capacity=1024)

    def refused(match, E=96, layout=lay, **kw):
        with pytest.raises(ValueError, match=match):
            PopulationTrainer(layout, E, **dict(ok, **kw))
    refused("members .* 1..64, not 0", members=0)
    refused("members .* 1..64, not 65", E=65 * 2, members=65)
    refused("members .* not 2.5", members=2.5)
    refused("multiple of members = 3, not 97", E=97)
    refused("multiple of members = 3, not 0", E=0)
    refused(r"\(E / members\) \* R = 5 must be even", E=15, layout=types.SimpleNamespace(R=1, P=300, device="cpu"))
    refused("batch must be even and > 0, not 255", batch=255)
    refused("batch must be even and > 0, not 0", batch=0)
    refused("replay_capacity must hold .* 128 rows .* not 100", replay_capacity=100)
    refused("learn_every .* not 0", learn_every=0)
    refused("lr must be a scalar or a sequence of members = 3 values, not 2", lr=(1e-3, 1e-4))
    refused("lr must be a finite number, not nan", lr=float("nan"))
    refused(r"lr must lie in \[0, inf\), not -0.001", lr=(1e-3, -1e-3, 1e-3))
    refused(r"gamma must lie in \[0, 1\], not 1.5", gamma=1.5)
    refused("epsilon must be a finite number, not inf", epsilon=float("inf"))
    refused(r"epsilon_decay must lie in \[0, 1\], not 2", epsilon_decay=(0.9, 2, 0.9))
    refused("target_every must be an integer >= 1, not 0", target_every=(2, 0, 5))
    refused("target_every must be an integer >= 1, not 2.0", target_every=2.0)
    refused("init_seeds must hold members = 3 seeds, not 2", init_seeds=[1, 2])
    refused("LayoutSet", layout=LayoutSet.__new__(LayoutSet))


def test_runner_broadcasts_its_arguments():
    sys.path.insert(0, os.path.join(ROOT, "dqn-marl_amd"))
    from Louvre_Evacuation.runners import train_pop
    b = train_pop.broadcast
    assert b("lr", "1e-3", 4, float, 0.5) == [1e-3] * 4
    assert b("lr", "1e-3, 3e-4,1e-4 ,3e-5", 4, float, 0.5) == [1e-3, 3e-4, 1e-4, 3e-5]
    assert b("lr", None, 3, float, 0.5) == [0.5] * 3
    assert b("target-every", "2,3", 2, int, 200) == [2, 3]
    with pytest.raises(ValueError, match="--lr: 2 values for 3 members"):
        b("lr", "1e-3,1e-4", 3, float, 0.5)
    with pytest.raises(ValueError, match="--target-every: cannot read '2.5' as int"):
        b("target-every", "2.5", 2, int, 200)
    args = train_pop.parse_args(["--members", "3", "--gamma", "0.99,0.95,0.9", "--seeds", "7", "--seed", "4"])
    hp = train_pop.member_hparams(args, dict(learning_rate=2e-4, target_update_freq=50))
    assert hp == dict(lr=[2e-4] * 3, gamma=[0.99, 0.95, 0.9], epsilon_decay=[0.9995] * 3, target_every=[50] * 3,
                      init_seeds=[7, 7, 7])
    assert train_pop.member_hparams(train_pop.parse_args(["--members", "2", "--seed", "4"]), {})["init_seeds"] == [4, 5]
    # the ranking: lowest death rate, then highest evacuation rate; no finished episode goes last
    rows = [dict(episodes=3, death_rate=0.2, evac_rate=0.5, return_mean=1.0),
            dict(episodes=3, death_rate=0.1, evac_rate=0.4, return_mean=2.0),
            dict(episodes=3, death_rate=0.1, evac_rate=0.6, return_mean=0.0),
            dict(episodes=0, death_rate=None, evac_rate=None, return_mean=None)]
    srow = train_pop.summary_row(10, rows)
    assert srow[0] == 10 and srow[-1] == 2 and len(srow) == len(train_pop.SUMMARY_COLUMNS)
    assert float(srow[1]) == 1.0 and float(srow[3]) == 0.0 and float(srow[4]) == 2.0  # reward mean, min, max
