"""The population's learner options without a GPU: PopulationTrainer's and per_member's
refusals, every -22 of the three device entries with its message (fake pointers, nothing launched), the
numpy restatement of evx_replay_sample_nstep_blocks (pop_opts_util, the reference of the GPU test) against
a float64 loop, and the stop causes on the very rings the GPU sampler test runs."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

import pop_opts_util as po
from golden_util import ROOT

FAKE = 0x1000  # a non-null address that is never dereferenced


def _m():
    from evacx import _lib
    return _lib


def _err():
    return _m().lib().evx_last_error().decode()


# ------------------------------------------------------------------ the trainer's refusals
def test_per_member_checks_the_options():
    from evacx.population import per_member
    assert per_member("loss", "huber", 3) == ["huber"] * 3
    assert per_member("loss", ("mse", "huber"), 2) == ["mse", "huber"]
    assert per_member("huber_delta", (0.5, 10), 2) == [0.5, 10.0]
    assert per_member("target_tau", (0, 0.005, 1), 3) == [0.0, 0.005, 1.0]
    assert per_member("n_step", (1, 3, 32), 3) == [1, 3, 32]
    for name, v, match in (("loss", "l1", "loss must be 'mse' or 'huber', not 'l1'"),
                           ("loss", ("mse", None), "loss must be 'mse' or 'huber', not None"),
                           ("loss", ("mse",), "loss must be a scalar or a sequence of members = 2 values, not 1"),
                           ("huber_delta", 0.0, "huber_delta must be > 0, not 0.0"),
                           ("huber_delta", (1.0, -2.0), "huber_delta must be > 0, not -2.0"),
                           ("huber_delta", float("inf"), "huber_delta must be a finite number, not inf"),
                           ("huber_delta", "1", "huber_delta must be a finite number, not '1'"),
                           ("target_tau", 1.5, r"target_tau must lie in \[0, 1\], not 1.5"),
                           ("target_tau", -0.1, r"target_tau must lie in \[0, 1\], not -0.1"),
                           ("target_tau", float("nan"), "target_tau must be a finite number, not nan"),
                           ("n_step", 0, "n_step must be an integer in 1..32, not 0"),
                           ("n_step", 33, "n_step must be an integer in 1..32, not 33"),
                           ("n_step", 2.0, "n_step must be an integer in 1..32, not 2.0"),
                           ("n_step", True, "n_step must be an integer in 1..32, not True")):
        with pytest.raises(ValueError, match=match):
            per_member(name, v, 2)


def test_population_trainer_refuses_bad_options_without_a_device():
    from evacx.population import PopulationTrainer, validate_population
    lay = types.SimpleNamespace(R=4, P=300, device="cpu")
    ok = dict(members=3, batch=256, replay_capacity=1024)  # E = 96: N = 128 rows per push

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            PopulationTrainer(lay, 96, **dict(ok, **kw))
    refused("loss must be 'mse' or 'huber', not 'l2'", loss=("mse", "l2", "huber"))
    refused("loss must be a scalar or a sequence of members = 3 values, not 2", loss=("mse", "huber"))
    refused("huber_delta must be > 0, not 0", huber_delta=0)
    refused("huber_delta must be a finite number, not nan", huber_delta=(1.0, float("nan"), 1.0))
    refused(r"target_tau must lie in \[0, 1\], not 2", target_tau=(0, 2, 0))
    refused("n_step must be an integer in 1..32, not 33", n_step=33)
    refused("n_step must be an integer in 1..32, not 1.5", n_step=(1, 1.5, 1))
    refused(r"n_step = 9 needs a replay_capacity of at least n_step \* N = 1152 slots .* not 1024", n_step=(1, 9, 8))
    refused("double_q must be a bool .* not 1", double_q=1)
    refused(r"double_q must be a bool .* not \[True, False, True\]", double_q=[True, False, True])
    assert validate_population(lay, 96, 3, 256, 1024, n_step=8) == 128  # 8 pushes of 128 rows just fit


# ------------------------------------------------------------------ the entries' refusals
def _ring(cap=512, **kw):
    f = dict(capacity=cap, s=FAKE, s2=FAKE, a=FAKE, r=FAKE, done=FAKE)
    f.update(kw)
    return _m().evx_replay(**f)


def _nstep(rp=True, size=512, B=256, nets=3, base=0, count=512, stride=128, n_step=(1, 3, 32), gamma=(0.99, 0.5, 1.0),
           null=None, ring=None):
    m = _m()
    ring = _ring() if ring is None else ring
    ns = None if n_step is None else (ctypes.c_int32 * len(n_step))(*n_step)
    gm = None if gamma is None else (ctypes.c_float * len(gamma))(*gamma)
    ptrs = [FAKE] * 8  # s, s2, a, r, done, gamma_row, len, idx_out
    if null is not None:
        ptrs[null] = None
    rc = m.lib().evx_replay_sample_nstep_blocks(ctypes.byref(ring) if rp else None, size, B, nets, 18, 0, base, count,
                                                stride, ns, gm, *ptrs, None)
    return rc, _err()


def test_replay_sample_nstep_blocks_refusals():
    T = "replay_sample_nstep_blocks: "
    assert "evx_replay_sample_nstep_blocks" in _m().SIGNATURES
    assert _nstep(rp=False) == (-22, T + "NULL argument")
    assert _nstep(n_step=None) == (-22, T + "NULL argument")
    assert _nstep(gamma=None) == (-22, T + "NULL argument")
    for i in range(6):  # s, s2, a, r, done, gamma_row (len and idx_out may be NULL)
        assert _nstep(null=i) == (-22, T + "NULL argument"), i
    assert _nstep(ring=_ring(r=None)) == (-22, T + "NULL ring array")
    assert _nstep(nets=0) == (-22, T + "nets must be 1..64")
    assert _nstep(nets=65, n_step=[1] * 65, gamma=[0.9] * 65) == (-22, T + "nets must be 1..64")
    assert _nstep(B=255) == (-22, T + "B must be even and >= 0")
    assert _nstep(B=-2) == (-22, T + "B must be even and >= 0")
    assert _nstep(size=0) == (-22, T + "size outside [1, capacity]")
    assert _nstep(size=513) == (-22, T + "size outside [1, capacity]")
    assert _nstep(size=200) == (-22, T + "sample larger than a ring's population (random.sample)")
    assert _nstep(count=-1) == (-22, T + "count outside [0, capacity]")
    assert _nstep(count=513) == (-22, T + "count outside [0, capacity]")
    assert _nstep(base=-1) == (-22, T + "base outside [0, capacity)")
    assert _nstep(base=512) == (-22, T + "base outside [0, capacity)")
    assert _nstep(stride=0) == (-22, T + "stride must be >= 1")
    assert _nstep(n_step=(1, 0, 3)) == (-22, T + "n_step must be 1..EVX_NSTEP_MAX (32)")
    assert _nstep(n_step=(1, 3, 33)) == (-22, T + "n_step must be 1..EVX_NSTEP_MAX (32)")
    assert _nstep(gamma=(0.99, float("nan"), 1.0)) == (-22, T + "gamma must be finite")
    assert _nstep(gamma=(float("inf"), 0.5, 1.0)) == (-22, T + "gamma must be finite")
    assert _nstep(B=0)[0] == 0  # nothing to draw: nothing launched
    assert _nstep(B=0, null=6)[0] == 0 and _nstep(B=0, null=7)[0] == 0


def _td(nets=3, deltas=(0.0, 0.5, 10.0), null=None, opt=True, B=256, ws_floats=64):
    m = _m()
    o = m.evx_td_opts(sel=FAKE, huber_delta=float("nan"), gamma_row=FAKE)  # (opt->huber_delta is not read)
    ptrs = dict(Q=FAKE, Qt=FAKE, act=FAKE, rew=FAKE, done=FAKE, dQ=FAKE, loss=FAKE, ws=FAKE)
    if null is not None:
        ptrs[null] = None
    dl = None if deltas is None else (ctypes.c_float * len(deltas))(*deltas)
    rc = m.lib().evx_td_loss_opt_nets(ptrs["Q"], ptrs["Qt"], 5, ptrs["act"], ptrs["rew"], ptrs["done"], 0.99, B, nets,
                                      None, ptrs["dQ"], ptrs["loss"], None, None, 0, ptrs["ws"], ws_floats,
                                      ctypes.byref(o) if opt else None, dl, None)
    return rc, _err()


def test_td_loss_opt_nets_refusals():
    T = "td_loss_opt_nets: "
    assert _td(deltas=None) == (-22, T + "NULL huber_delta")
    assert _td(nets=0) == (-22, T + "nets must be 1..64")
    assert _td(nets=65, deltas=[1.0] * 65) == (-22, T + "nets must be 1..64")
    assert _td(deltas=(0.0, -0.5, 1.0)) == (-22, T + "huber_delta must be finite and >= 0")
    assert _td(deltas=(float("nan"), 0.5, 1.0)) == (-22, T + "huber_delta must be finite and >= 0")
    assert _td(deltas=(0.0, 0.5, float("inf"))) == (-22, T + "huber_delta must be finite and >= 0")
    for name in ("Q", "Qt", "act", "rew", "done", "dQ", "loss"):
        assert _td(null=name) == (-22, T + "NULL argument"), name
    # what evx_td_loss_opt refuses, with its text
    assert _td(null="ws") == (-22, "td_loss: workspace smaller than evx_td_loss_ws_floats")
    assert _td(ws_floats=2) == (-22, "td_loss: workspace smaller than evx_td_loss_ws_floats")
    assert _td(B=0)[0] == 0 and _td(B=0, opt=False)[0] == 0  # nothing to do: nothing launched


def _polyak(nets=3, tau=(0.0, 0.005, 1.0), omt=(1.0, 0.995, 0.0), null=None):
    m = _m()
    ptrs = [FAKE, FAKE] + [None if tau is None else (ctypes.c_float * len(tau))(*tau),
                           None if omt is None else (ctypes.c_float * len(omt))(*omt)] + [FAKE] * 9
    for i in ([] if null is None else null):
        ptrs[i] = None
    rc = m.lib().evx_qmlp_polyak_pack3_g(*ptrs, nets, None)
    return rc, _err()


def test_polyak_pack3_g_refusals():
    T = "qmlp_polyak_pack3_g: "
    assert _polyak(tau=None) == (-22, T + "NULL argument")
    assert _polyak(omt=None) == (-22, T + "NULL argument")
    for i in (0, 1, 4, 5, 6, 7, 8):  # p, t, w1b, w1l, b1c, w2b, w2l
        assert _polyak(null=[i]) == (-22, T + "NULL argument"), i
    assert _polyak(nets=0) == (-22, T + "nets must be 1..64")
    assert _polyak(nets=65, tau=[0.1] * 65, omt=[0.9] * 65) == (-22, T + "nets must be 1..64")
    assert _polyak(null=[11]) == (-22, T + "w1o and w1ol go together")
    assert _polyak(null=[12]) == (-22, T + "w1o and w1ol go together")
    assert _polyak(null=[9]) == (-22, T + "w2t and w2tl go together")
    assert _polyak(tau=(0.0, 1.5, 1.0)) == (-22, T + "tau must lie in [0, 1]")
    assert _polyak(tau=(-0.1, 0.5, 1.0)) == (-22, T + "tau must lie in [0, 1]")
    assert _polyak(tau=(0.0, float("nan"), 1.0)) == (-22, T + "tau must lie in [0, 1]")
    assert _polyak(omt=(1.0, float("inf"), 0.0)) == (-22, T + "one_minus_tau must be finite")


# ------------------------------------------------------------------ the restatement
CASES = [(cap, state, K) for cap in (512, 600) for state in ("part", "full", "wrapped") for K in (1, 3)]


@pytest.mark.parametrize("cap,state,K", CASES)
def test_restatement_matches_a_float64_loop(cap, state, K):
    """Rewards that are multiples of 2^-6 below 4 and gamma = 0.5: a ring holds at most 5 pushes, so a chain
    has at most 5 links and every partial sum is a multiple of 2^-10 below 8 -- 13 bits, exact in f32 (and
    in float64): the f32 restatement must equal the float64 loop, whatever n_step asks for."""
    ring, size, pos = po.synthetic_rings(K, cap, po.PUSHES[cap][state], exact=True)
    n_step = po.MEMBER_OPTS[K][0]
    out = po.np_sample_nstep_blocks(ring, size, pos, 190, 18, 5 * K * 190, n_step, [0.5] * K, po.N_ROWS)
    base = (pos - size) % cap
    for k in range(K):
        assert len(set(out["idx"][k].tolist())) == 190 and out["idx"][k].max() < size  # without replacement
        R, G, L = po.naive_chain_f64(ring["r"][k], ring["done"][k], out["idx"][k], base, size, po.N_ROWS, n_step[k], 0.5)
        assert L.max() <= 5
        assert np.array_equal(out["r"][k].astype(np.float64), R), k
        assert np.array_equal(out["gamma_row"][k].astype(np.float64), G), k
        assert np.array_equal(out["len"][k], L), k


@pytest.mark.parametrize("cap,state,K", CASES)
def test_restatement_with_n_step_1_is_the_plain_sampler(cap, state, K):
    ring, size, pos = po.synthetic_rings(K, cap, po.PUSHES[cap][state])
    gam = po.GAMMAS[:K]
    out = po.np_sample_nstep_blocks(ring, size, pos, 256, 18, 0, [1] * K, gam, po.N_ROWS)
    idx = po.np_block_draws(size, 256, K, 18, 0)
    assert np.array_equal(out["idx"], idx) and (out["len"] == 1).all()
    for k in range(K):
        for name in ("s", "s2", "a", "r", "done"):
            assert np.array_equal(out[name][k], ring[name][k][idx[k]]), (name, k)
        assert (out["gamma_row"][k] == np.float32(gam[k])).all()


@pytest.mark.parametrize("B", [190, 256, 258])
@pytest.mark.parametrize("cap,state,K", CASES)
def test_every_stop_cause_occurs_on_the_gpu_test_inputs(cap, state, K, B):
    """On the rings, draws and options of tests/test_population_opts_gpu.py's sampler cases: some chain
    reaches its member's n_step (> 1), some chain is cut by a done, some by the end of the range."""
    ring, size, pos = po.synthetic_rings(K, cap, po.PUSHES[cap][state])
    n_step, gam = po.MEMBER_OPTS[K]
    out = po.np_sample_nstep_blocks(ring, size, pos, B, 18, 3 * K * B, n_step, gam, po.N_ROWS)
    full, by_done, by_range = po.stop_causes(out["len"], out["done"], n_step)
    assert full > 0 and by_done > 0 and by_range > 0, (full, by_done, by_range)
    base = (pos - size) % cap
    for k in range(K):  # nothing else ends a chain early
        cut = (out["len"][k] < n_step[k]) & (out["done"][k] == 0)
        d0 = (out["idx"][k] - base) % cap
        assert (d0[cut] + out["len"][k][cut].astype(np.int64) * po.N_ROWS >= size).all()


# ------------------------------------------------------------------ the runner
def test_runner_reads_the_option_flags_and_config_keys(capsys):
    sys.path.insert(0, os.path.join(ROOT, "dqn-marl_amd"))
    from Louvre_Evacuation.runners import train_pop
    with pytest.raises(SystemExit) as e:
        train_pop.parse_args(["--help"])
    text = capsys.readouterr().out
    assert e.value.code == 0 and all(f in text for f in ("--double-q", "--loss", "--huber-delta", "--target-tau", "--n-step"))
    a = train_pop.parse_args(["--members", "3"])
    assert train_pop.member_options(a, {}) == dict(double_q=False, loss=["mse"] * 3, huber_delta=[1.0] * 3,
                                                   target_tau=[0.0] * 3, n_step=[1] * 3)
    cfg = dict(double_dqn=True, loss="huber", huber_delta=2.0, target_tau=0.01, n_step=3)
    assert train_pop.member_options(a, cfg) == dict(double_q=True, loss=["huber"] * 3, huber_delta=[2.0] * 3,
                                                    target_tau=[0.01] * 3, n_step=[3] * 3)
    a = train_pop.parse_args(["--members", "3", "--double-q", "--loss", "mse,huber,huber", "--huber-delta", "1,0.5,10",
                              "--target-tau", "0,0.01,0", "--n-step", "1,3,2"])
    assert train_pop.member_options(a, cfg) == dict(double_q=True, loss=["mse", "huber", "huber"],
                                                    huber_delta=[1.0, 0.5, 10.0], target_tau=[0.0, 0.01, 0.0],
                                                    n_step=[1, 3, 2])
    for argv, match in ((["--loss", "l1"], "loss must be 'mse' or 'huber'"), (["--n-step", "0"], "n_step must be an integer"),
                        (["--n-step", "1,2"], "--n-step: 2 values for 3 members"),
                        (["--target-tau", "1.5"], "target_tau must lie in"), (["--huber-delta", "0"], "huber_delta must be > 0")):
        with pytest.raises(ValueError, match=match):
            train_pop.member_options(train_pop.parse_args(["--members", "3"] + argv), {})
