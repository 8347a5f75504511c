"""Learner options for per-robot and QMIX nets without a device: the numpy restatement of
evx_replay_sample_nstep_agents (also the reference of tests/test_replay_marl_nstep_gpu.py and
tests/test_marl_opts_gpu.py) against a naive float64 chain, the argument checks of the two new
entries before any launch, the trainer's pure validation function and the runner's flags."""
import ctypes as C
import math

import numpy as np
import pytest

import marl_opts_util as mu
from test_nstep_cpu import naive_f64


def _range_and_batch(ring, nets):
    base, count = ring.live_range()
    return base, count, ring.size // nets  # every slot of every agent once


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("nets", mu.NETS)
def test_restatement_matches_a_naive_float64_chain(nets, joint):
    """Integer rewards of magnitude <= 3 and gamma = 0.5: every partial sum is a multiple of 2^-4
    below 8, exact in f32, so the f32 restatement must equal the float64 loop."""
    stride = mu.stride_of(nets)
    for state in mu.STATES:
        ring = mu.ring_fixture(nets, state, integer_rewards=True)
        base, count, B = _range_and_batch(ring, nets)
        for n in mu.NSTEPS:
            out = mu.np_sample_nstep_agents(ring, B, nets, joint, mu.SEED, mu.OFFSET, base, count, stride, n, 0.5)
            R64, G64 = naive_f64(ring.r, ring.done, out["idx"], base, count, stride, n, 0.5)
            assert np.array_equal(out["r"].astype(np.float64), R64), (state, n)
            assert np.array_equal(out["gamma_row"].astype(np.float64), G64), (state, n)
            assert np.array_equal(out["gamma_row"], np.float32(0.5) ** out["len"])
            # rows [g B, (g + 1) B) are agent g's slots, each once, and s / a are the drawn slot's
            idx = out["idx"].reshape(nets, B)
            for g in range(nets):
                assert (idx[g] % nets == g).all() and len(set(idx[g].tolist())) == B
            assert np.array_equal(out["s"], ring.s[out["idx"]]) and np.array_equal(out["a"], ring.a[out["idx"]])
            last = (out["idx"] + (out["len"] - 1).astype(np.int64) * stride) % mu.CAP
            assert np.array_equal(out["s2"], ring.s2[last]) and np.array_equal(out["done"], ring.done[last])
            if n == 1:
                plain = ring.sample_joint(B, nets, mu.SEED, mu.OFFSET) if joint else \
                    ring.sample_agents(B, nets, mu.SEED, mu.OFFSET)
                for k in ("s", "s2", "a", "r", "done"):
                    assert np.array_equal(out[k], plain[k]), k
                assert (out["len"] == 1).all() and (out["gamma_row"] == np.float32(0.5)).all()
            if joint:  # one draw: the same env-steps for every agent, so one chain length
                assert (idx // nets == idx[0] // nets).all()
                for k in ("len", "r", "done", "gamma_row"):
                    rows = out[k].reshape(nets, B)
                    assert (rows == rows[0]).all(), k


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("nets", mu.NETS)
def test_every_row_kind_occurs_on_the_fixture(nets, joint):
    """On the fixture the GPU test runs (f32 rewards): rows ending on a done, on the end of the
    range and at full length, and rows whose successor wrapped past the end of the ring."""
    stride = mu.stride_of(nets)
    tot = np.zeros(4, np.int64)
    for state in mu.STATES:
        ring = mu.ring_fixture(nets, state)
        base, count, B = _range_and_batch(ring, nets)
        for n in mu.NSTEPS[1:]:
            out = mu.np_sample_nstep_agents(ring, B, nets, joint, mu.SEED, mu.OFFSET, base, count, stride, n, 0.99)
            kinds = np.array(mu.row_kinds(out, base, count, stride, n))
            if state != "wrapped":
                assert kinds[3] == 0  # base 0: no chain leaves the ring's end
            tot += kinds
    by_done, by_range, full, wrapped = tot
    assert by_done > 0 and by_range > 0 and full > 0 and wrapped > 0, tot


# ------------------------------------------------------------------ the entries' argument checks
def _host_ring(cap=mu.CAP):
    from evacx import _lib
    host = dict(s=np.zeros((cap, 8), np.int32), s2=np.zeros((cap, 8), np.int32), a=np.zeros(cap, np.int32),
                r=np.zeros(cap, np.float32), done=np.zeros(cap, np.uint8))
    return _lib.evx_replay(capacity=cap, **{k: v.ctypes.data for k, v in host.items()}), host


def _sample(L, ring, out, **kw):
    a = dict(rp=C.byref(ring), size=64, B=4, nets=2, joint=0, seed=1, offset=0, base=0, count=64, stride=4, n_step=3,
             gamma=0.99, s=out["s"].ctypes.data, s2=out["s2"].ctypes.data, a=out["a"].ctypes.data,
             r=out["r"].ctypes.data, done=out["done"].ctypes.data, gamma_row=out["g"].ctypes.data, len=None,
             idx_out=None)
    a.update(kw)
    return L.evx_replay_sample_nstep_agents(*[a[k] for k in (
        "rp", "size", "B", "nets", "joint", "seed", "offset", "base", "count", "stride", "n_step", "gamma", "s", "s2",
        "a", "r", "done", "gamma_row", "len", "idx_out")], None)


def test_replay_sample_nstep_agents_validates_before_any_launch():
    from evacx import _lib
    L = _lib.lib()
    assert "evx_replay_sample_nstep_agents" in _lib.SIGNATURES
    ring, host = _host_ring()
    out = dict(s=np.zeros((8, 8), np.int32), s2=np.zeros((8, 8), np.int32), a=np.zeros(8, np.int32),
               r=np.zeros(8, np.float32), done=np.zeros(8, np.uint8), g=np.zeros(8, np.float32))
    no_s2 = _lib.evx_replay(capacity=mu.CAP, s=host["s"].ctypes.data, a=host["a"].ctypes.data,
                            r=host["r"].ctypes.data, done=host["done"].ctypes.data)
    bad = [
        # what evx_replay_nstep refuses about base / count / stride / n_step / gamma
        (dict(n_step=0), b"n_step must be 1.."), (dict(n_step=33), b"n_step must be 1.."),
        (dict(stride=0), b"stride must be >= 1"), (dict(count=mu.CAP + 1), b"count must lie in [0, capacity]"),
        (dict(count=-1), b"count must lie in [0, capacity]"), (dict(base=mu.CAP), b"base must lie in [0, capacity)"),
        (dict(base=-1), b"base must lie in [0, capacity)"), (dict(gamma=math.nan), b"gamma must be finite"),
        (dict(gamma=math.inf), b"gamma must be finite"),
        # what the two samplers refuse
        (dict(rp=None), b"NULL argument"), (dict(s=None), b"NULL argument"), (dict(s2=None), b"NULL argument"),
        (dict(a=None), b"NULL argument"), (dict(r=None), b"NULL argument"), (dict(done=None), b"NULL argument"),
        (dict(nets=0), b"nets must be 1..65535"), (dict(nets=65536), b"nets must be 1..65535"),
        (dict(nets=5, size=60), b"capacity must be a multiple of nets"),
        (dict(size=63), b"size must be a positive multiple of nets"), (dict(size=0), b"size must be a positive"),
        (dict(size=mu.CAP + 2), b"size must be a positive multiple of nets within the capacity"),
        (dict(B=33), b"sample larger than an agent's population"),
        (dict(B=33, joint=1), b"sample larger than the population"),
        # its own
        (dict(gamma_row=None), b"NULL argument"), (dict(rp=C.byref(no_s2)), b"NULL ring array"),
        (dict(rp=C.byref(_lib.evx_replay(capacity=0))), b"bad ring"),
        (dict(rp=C.byref(_lib.evx_replay(capacity=-4))), b"bad ring"),
    ]
    for kw, word in bad:
        assert _sample(L, ring, out, **kw) == -22, kw
        msg = L.evx_q_last_error()
        assert msg.startswith(b"replay_sample_nstep_agents") and word in msg, (kw, msg)
    assert _sample(L, ring, out, B=0) == 0  # nothing to do is not an error, and launches nothing
    assert _sample(L, ring, out, B=-3) == 0


def _qmix(L, bufs, opt="default", **kw):
    from evacx.qmlp import td_opts
    p = {k: v.ctypes.data for k, v in bufs.items()}
    a = dict(Q=p["Q"], Qt=p["Qt"], A=5, act=p["act"], rew=p["rew"], done=p["done"], gamma=0.99, B=4, n=2,
             mix=p["mix"], mix_t=p["mix_t"], dQ=p["dQ"], mix_grad=p["grad"], loss=p["loss"], part=p["part"],
             zero=None, nzero=0, td_abs=None)
    hub = kw.pop("huber_delta", 0.0)
    a.update(kw)
    o = None if opt is None else C.byref(td_opts(huber_delta=hub))
    return L.evx_qmix_loss_opt(*[a[k] for k in ("Q", "Qt", "A", "act", "rew", "done", "gamma", "B", "n", "mix", "mix_t",
                                                "dQ", "mix_grad", "loss", "part", "zero", "nzero")], o, a["td_abs"],
                               None)


def test_qmix_loss_opt_validates_before_any_launch():
    from evacx import _lib
    L = _lib.lib()
    assert "evx_qmix_loss_opt" in _lib.SIGNATURES
    f = np.float32
    bufs = dict(Q=np.zeros(40, f), Qt=np.zeros(40, f), act=np.zeros(8, np.int32), rew=np.zeros(4, f),
                done=np.zeros(4, np.uint8), mix=np.zeros(200, f), mix_t=np.zeros(200, f), dQ=np.zeros(40, f),
                grad=np.zeros(200, f), loss=np.zeros(1, f), part=np.zeros(400, f))
    bad = [
        # everything evx_qmix_loss refuses
        (dict(n=0), b"agents"), (dict(n=17), b"agents"), (dict(A=0), b"actions"), (dict(A=65), b"actions"),
    ] + [({k: None}, b"NULL") for k in ("Q", "Qt", "act", "rew", "done", "mix", "mix_t", "dQ", "mix_grad", "loss",
                                        "part")] + [
        # its own
        (dict(huber_delta=-1.0), b"huber_delta"), (dict(huber_delta=math.nan), b"huber_delta"),
        (dict(huber_delta=math.inf), b"huber_delta"), (dict(gamma=math.nan), b"gamma"),
        (dict(gamma=-math.inf), b"gamma"),
    ]
    for kw, word in bad:
        assert _qmix(L, bufs, **kw) == -22, kw
        msg = L.evx_qmix_last_error()
        assert msg.startswith(b"qmix_loss_opt") and word in msg, (kw, msg)
    assert _qmix(L, bufs, opt=None, n=17) == -22  # a NULL opt is checked like any other
    for B in (0, -1):  # nothing to do: 0, nothing written (not even with arguments it would refuse)
        assert _qmix(L, bufs, B=B) == 0 and _qmix(L, bufs, B=B, n=99, huber_delta=-1.0) == 0
    assert all(not v.any() for v in bufs.values())


# ------------------------------------------------------------------ the trainer's validation
def test_validate_nets_options():
    from evacx.qnet import validate_nets_options as v
    ok = dict(R=4, E=64, batch=64, replay_capacity=4096, agent_options=True)
    for nets in ("per_robot", "qmix"):  # VecTrainer (agent_options=False) keeps its refusals
        v(nets, R=4, E=64, batch=64, replay_capacity=4096)
        with pytest.raises(ValueError, match="nets='shared'"):
            v(nets, R=4, E=64, batch=64, replay_capacity=4096, td_options=True)
        with pytest.raises(ValueError, match="nets='shared'"):
            v(nets, R=4, E=64, batch=64, replay_capacity=4096, n_step=2)
        v(nets, td_options=True, n_step=2, **ok)
    for nets in ("shared", "per_robot", "qmix"):
        v(nets, **ok)
        v(nets, n_step=3, **ok)  # n-step returns go with every nets mode now
        v(nets, n_step=16, **ok)  # 16 * 64 * 4 = 4096: a chain just fits
        with pytest.raises(ValueError, match="n_step"):
            v(nets, n_step=17, **ok)
        with pytest.raises(ValueError, match="groups"):
            v(nets, n_step=2, groups=2, **ok)
        for bad in (0, 33, 2.0, True, None):
            with pytest.raises(ValueError, match="n_step"):
                v(nets, n_step=bad, **ok)
    with pytest.raises(ValueError, match="nets must be"):
        v("vdn", **ok)
    for nets in ("per_robot", "qmix"):  # the per-robot conditions stay
        for kw in (dict(kind="conv"), dict(precision="bf16"), dict(groups=2), dict(lagged_learn=True),
                   dict(replay="prioritized"), dict(per_env_layouts=True), dict(grad_hook=True)):
            with pytest.raises(ValueError, match="per_robot nets: MLP"):
                v(nets, **dict(ok, **kw))
        with pytest.raises(ValueError, match="multiple of 2 R"):
            v(nets, **dict(ok, batch=68))
        with pytest.raises(ValueError, match="multiple of 2 R"):
            v(nets, **dict(ok, replay_capacity=4098))
    v("shared", kind="conv", precision="bf16", groups=2, lagged_learn=True, replay="prioritized", **ok)


def test_trainer_checks_options_before_it_touches_the_device():
    """MultiAgentTrainer runs the pure checks first (a layout stand-in without a device is enough);
    VecTrainer itself keeps refusing the options for per-robot and QMIX nets."""
    from types import SimpleNamespace

    from evacx.trainer import MultiAgentTrainer, VecTrainer
    with pytest.raises(ValueError, match="nets must be 'per_robot' or 'qmix'"):
        MultiAgentTrainer(SimpleNamespace(R=4), 64, nets="shared")
    for nets in ("per_robot", "qmix"):
        for opt in (dict(double_q=True), dict(loss="huber"), dict(huber_delta=2.0), dict(target_tau=0.01)):
            with pytest.raises(ValueError, match="nets='shared'.*MultiAgentTrainer"):
                VecTrainer(SimpleNamespace(R=4), 64, batch=64, replay_capacity=4096, nets=nets, **opt)
        with pytest.raises(ValueError, match="n_step > 1 needs nets='shared'"):
            VecTrainer(SimpleNamespace(R=4), 64, batch=64, replay_capacity=4096, nets=nets, n_step=2)
    lay = SimpleNamespace(R=4)
    for nets in ("per_robot", "qmix"):
        with pytest.raises(ValueError, match="huber_delta"):
            MultiAgentTrainer(lay, 64, batch=64, replay_capacity=4096, nets=nets, loss="huber", huber_delta=-1.0)
        with pytest.raises(ValueError, match="target_tau"):
            MultiAgentTrainer(lay, 64, batch=64, replay_capacity=4096, nets=nets, target_tau=1.0)
        with pytest.raises(ValueError, match="n_step"):
            MultiAgentTrainer(lay, 64, batch=64, replay_capacity=4096, nets=nets, n_step=17)
        with pytest.raises(ValueError, match="multiple of 2 R"):
            MultiAgentTrainer(lay, 64, batch=68, replay_capacity=4096, nets=nets, double_q=True)


def test_grouped_qmix_checks_its_options_without_a_device():
    from types import SimpleNamespace

    from evacx.qgroup import GroupedQMix
    qm = GroupedQMix.__new__(GroupedQMix)
    qm.A = SimpleNamespace(G=2)
    for bad in (-1.0, math.nan, math.inf, "1"):
        with pytest.raises(ValueError, match="huber_delta"):
            qm(None, None, None, None, None, None, 8, huber_delta=bad)
    import torch
    with pytest.raises(ValueError, match="gamma_row"):
        qm(None, None, None, None, None, None, 8, gamma_row=torch.zeros(7))
    with pytest.raises(ValueError, match="gamma_row"):
        qm(None, None, None, None, None, None, 8, gamma_row=torch.zeros(8, dtype=torch.float64))


# ------------------------------------------------------------------ the runner
def test_train_vec_sizes_the_ring_for_any_robot_count():
    """batch_and_capacity: for per-robot and QMIX nets the batch is a multiple of 2 R and the capacity a
    multiple of R at every robot count (3, 5, 6, 7 are no powers of two), and the trainer's checks take
    the pair; the shared net keeps its power-of-two ring."""
    from evacx.qnet import validate_nets_options
    from Louvre_Evacuation.runners import train_vec as tv
    assert tv.batch_and_capacity(256, 50000, 4096, 1, 1, "shared") == (256, 1 << 16)
    assert tv.batch_and_capacity(256, 50000, 4096, 3, 1, "shared") == (256, 1 << 16)
    assert tv.batch_and_capacity(256, 50000, 4096, 2, 1, "qmix") == (256, 1 << 16)  # powers of two: as before
    assert tv.batch_and_capacity(256, 50000, 4096, 3, 1, "per_robot") == (258, 65538)
    for nets in ("per_robot", "qmix"):
        for R in range(2, 17):
            for n_step in (1, 3, 32):
                for envs in (2, 64, 4096):
                    b, c = tv.batch_and_capacity(256, 50000, envs, R, n_step, nets)
                    need = max(50000, 4 * b, max(2, n_step) * envs * R)
                    assert b >= 256 and b % (2 * R) == 0 and c % R == 0 and need <= c < 2 * need + R, (R, b, c)
                    validate_nets_options(nets, R=R, E=envs, batch=b, replay_capacity=c, n_step=n_step,
                                          td_options=True, agent_options=True)


def test_train_vec_nets_and_robots_flags(capsys):
    from Louvre_Evacuation.runners import train_vec as tv
    with pytest.raises(SystemExit) as e:
        tv.parse_args(["--help"])
    out = capsys.readouterr().out
    assert e.value.code == 0 and "--nets" in out and "--robots" in out
    a = tv.parse_args([])
    assert (a.robots, a.nets) == (1, "shared") and tv.nets_option(a) == "shared"
    assert tv.nets_option(tv.parse_args(["--robots", "3"])) == "shared"
    for nets in ("per_robot", "qmix"):
        a = tv.parse_args(["--nets", nets, "--robots", "2", "--double-q", "--loss", "huber", "--n-step", "3",
                           "--target-tau", "0.01"])
        assert tv.nets_option(a) == nets
        assert tv.td_options(a, {}) == dict(double_q=True, loss="huber", huber_delta=1.0, target_tau=0.01)
        assert tv.n_step_option(a, {}) == 3
        # the optional agent: keys apply to these modes as to the shared net
        b = tv.parse_args(["--nets", nets, "--robots", "2"])
        assert tv.td_options(b, dict(double_dqn=True, target_tau=0.05))["double_q"] is True
        assert tv.n_step_option(b, dict(n_step=4)) == 4
        with pytest.raises(ValueError, match="--robots >= 2"):
            tv.nets_option(tv.parse_args(["--nets", nets]))
        with pytest.raises(ValueError, match="--qnet mlp"):
            tv.nets_option(tv.parse_args(["--nets", nets, "--robots", "2", "--qnet", "conv"]))
    with pytest.raises(ValueError, match="--robots"):
        tv.nets_option(tv.parse_args(["--robots", "0"]))
    with pytest.raises(ValueError, match="learn-stats"):
        tv.nets_option(tv.parse_args(["--nets", "qmix", "--robots", "2", "--learn-stats"]))
    assert tv.nets_option(tv.parse_args(["--nets", "per_robot", "--robots", "2", "--learn-stats"])) == "per_robot"
    with pytest.raises(SystemExit):
        tv.parse_args(["--nets", "vdn"])
    capsys.readouterr()
