"""The population's learner options on the GPU (evacx.population): the three device entries
against the single-net pieces they replace, bit for bit (torch.equal), and ``PopulationTrainer`` with
per-member Huber, Polyak and n-step and population-wide Double-Q against
``pop_opts_util.SlowPopulationOpts`` -- the same K members stepped one by one with ``Learner`` and
``Replay``. Shapes: tests/test_population_gpu.py's."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pop_opts_util as po
import pop_util as pu

pytestmark = pytest.mark.gpu
PAD = 256  # sentinel elements on both sides of every output


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _padded(n, dtype, sent):
    """(whole, view): n elements with PAD sentinel elements before and behind."""
    whole = torch.full((n + 2 * PAD,), sent, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + n]


def _pads_intact(whole, n, sent):
    return bool((whole[:PAD] == sent).all()) and bool((whole[PAD + n:] == sent).all())


# ------------------------------------------------------------------ a. the sampler
_OUT = (("s", 8, torch.int32, -1), ("s2", 8, torch.int32, -2), ("a", 1, torch.int32, -3), ("r", 1, torch.float32, -4.0),
        ("done", 1, torch.uint8, 7), ("gamma_row", 1, torch.float32, -5.0), ("nlen", 1, torch.int32, -6),
        ("idx", 1, torch.int64, -7))


def _device_rings(ring, size, pos):
    """(BlockReplay, [Replay per ring]) holding the host rings."""
    from evacx.population import BlockReplay
    from evacx.trainer import Replay
    K, cap = ring["r"].shape
    br = BlockReplay(K, cap, "cuda")
    seps = [Replay(cap, "cuda") for _ in range(K)]
    for name in ("s", "s2", "a", "r", "done"):
        getattr(br, name).copy_(torch.from_numpy(ring[name].reshape(-1)))
        for k, rp in enumerate(seps):
            getattr(rp, name).copy_(torch.from_numpy(ring[name][k].reshape(-1)))
    for rp in [br] + seps:
        rp.size, rp.pos = size, pos
    return br, seps


def _sample_nstep(br, B, seed, offset, n_step, gamma):
    K = br.K
    whole, out = {}, {}
    for name, per, dt, sent in _OUT:
        whole[name], out[name] = _padded(K * B * per, dt, sent)
    br.sample_nstep(B, seed, offset, n_step, gamma, po.N_ROWS, out)
    torch.cuda.synchronize()
    for name, per, dt, sent in _OUT:
        assert _pads_intact(whole[name], K * B * per, sent), name
    return out


@pytest.mark.parametrize("B", [190, 256, 258])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("state", ["part", "full", "wrapped"])
@pytest.mark.parametrize("cap", [512, 600])
def test_sample_nstep_blocks_equals_separate_rings(cap, state, K, B):
    """evx_replay_sample_nstep_blocks against K Replay.sample + Replay.nstep calls and against the numpy
    restatement: all eight outputs by torch.equal, 256 sentinels on both sides of each, two runs bit-equal,
    every n_step = 1 the plain blocked sampler. N = 128 rows per push; members (n_step, gamma) = (1, 0.99),
    (3, 0.5), (32, 1.0), K = 1 the middle one (pop_opts_util.MEMBER_OPTS). On len: some chain reaches its
    member's n_step, some is cut by a done, some by the end of the range."""
    _need_gpu()
    ring, size, pos = po.synthetic_rings(K, cap, po.PUSHES[cap][state])
    n_step, gam = po.MEMBER_OPTS[K]
    seed, offset = 18, 3 * K * B
    br, seps = _device_rings(ring, size, pos)
    assert br.live_range() == seps[0].live_range() == ((pos - size) % cap, size)
    out = _sample_nstep(br, B, seed, offset, n_step, gam)
    again = _sample_nstep(br, B, seed, offset, n_step, gam)
    for name, per, dt, sent in _OUT:
        assert torch.equal(out[name], again[name]), name
    # K separate rings: the draw with its slots, then the chain
    for k, rp in enumerate(seps):
        o = dict(s=torch.zeros(B * 8, dtype=torch.int32, device="cuda"),
                 s2=torch.zeros(B * 8, dtype=torch.int32, device="cuda"),
                 a=torch.zeros(B, dtype=torch.int32, device="cuda"), r=torch.zeros(B, device="cuda"),
                 done=torch.zeros(B, dtype=torch.uint8, device="cuda"),
                 idx=torch.zeros(B, dtype=torch.int64, device="cuda"), gamma_row=torch.zeros(B, device="cuda"),
                 nlen=torch.zeros(B, dtype=torch.int32, device="cuda"))
        rp.sample(B, seed, offset + k * B, o)
        base, count = rp.live_range()
        rp.nstep(o["idx"], B, base, count, po.N_ROWS, n_step[k], gam[k], o)
        torch.cuda.synchronize()
        for name, per, dt, sent in _OUT:
            assert torch.equal(out[name][k * B * per:(k + 1) * B * per], o[name]), (name, k)
    # the numpy restatement
    ref = po.np_sample_nstep_blocks(ring, size, pos, B, seed, offset, n_step, gam, po.N_ROWS)
    for name, per, dt, sent in _OUT:
        want = torch.from_numpy(ref["len" if name == "nlen" else name].reshape(-1))
        assert torch.equal(out[name].cpu(), want), name
    L, D = out["nlen"].cpu().numpy().reshape(K, B), out["done"].cpu().numpy().reshape(K, B)
    full, by_done, by_range = po.stop_causes(L, D, n_step)
    assert full > 0 and by_done > 0 and by_range > 0, (full, by_done, by_range)
    # every n_step = 1: evx_replay_sample_blocks bit for bit, gamma_row = gamma[k], len = 1
    one = _sample_nstep(br, B, seed, offset, [1] * K, gam)
    plain = {name: torch.zeros(K * B * per, dtype=dt, device="cuda") for name, per, dt, sent in _OUT[:5]}
    br.sample(B, seed, offset, plain)
    torch.cuda.synchronize()
    for name in plain:
        assert torch.equal(one[name], plain[name]), name
    assert bool((one["nlen"] == 1).all())
    assert torch.equal(one["gamma_row"].cpu(), torch.tensor(gam, dtype=torch.float32).repeat_interleave(B))
    assert torch.equal(one["idx"], out["idx"])


def test_sample_nstep_optional_outputs_and_stride_beyond_the_ring():
    """len and idx_out may be left out; a stride beyond the ring stands for the capacity: no slot has a
    successor inside the range, every chain is its own row."""
    _need_gpu()
    K, cap, B = 3, 512, 190
    ring, size, pos = po.synthetic_rings(K, cap, 7)
    br, _ = _device_rings(ring, size, pos)
    out = {name: torch.zeros(K * B * per, dtype=dt, device="cuda") for name, per, dt, sent in _OUT[:6]}
    br.sample_nstep(B, 18, 0, po.NSTEPS, po.GAMMAS, po.N_ROWS, out)
    full = _sample_nstep(br, B, 18, 0, po.NSTEPS, po.GAMMAS)
    torch.cuda.synchronize()
    for name in out:
        assert torch.equal(out[name], full[name]), name
    big = {name: torch.zeros(K * B * per, dtype=dt, device="cuda") for name, per, dt, sent in _OUT}
    br.sample_nstep(B, 18, 0, po.NSTEPS, po.GAMMAS, 1 << 40, big)
    plain = {name: torch.zeros(K * B * per, dtype=dt, device="cuda") for name, per, dt, sent in _OUT[:5]}
    br.sample(B, 18, 0, plain)
    torch.cuda.synchronize()
    assert bool((big["nlen"] == 1).all())
    for name in plain:
        assert torch.equal(big[name], plain[name]), name
    with pytest.raises(ValueError, match="n_step and gamma must hold 3"):
        br.sample_nstep(B, 18, 0, (1, 2), po.GAMMAS, po.N_ROWS, big)
    with pytest.raises(ValueError, match="out\\['gamma_row'\\] holds"):
        br.sample_nstep(B, 18, 0, po.NSTEPS, po.GAMMAS, po.N_ROWS, dict(big, gamma_row=big["gamma_row"][:B]))


# ------------------------------------------------------------------ b. the TD loss with a delta per net
TD_K, TD_DELTAS, TD_SCALE = 3, (0.0, 0.5, 10.0), (1.0, 0.3, 6.0)


def _td_inputs(B):
    """Q, Qt, r of net k drawn at TD_SCALE[k], so that |d| lies on both sides of net k's delta."""
    g = torch.Generator().manual_seed(B)
    sc = torch.tensor(TD_SCALE).repeat_interleave(B)
    return dict(Q=(torch.randn(TD_K * B, 5, generator=g) * sc[:, None]).cuda(),
                Qt=(torch.randn(TD_K * B, 5, generator=g) * sc[:, None]).cuda(),
                a=torch.randint(0, 5, (TD_K * B,), generator=g, dtype=torch.int32).cuda(),
                r=(torch.randn(TD_K * B, generator=g) * sc).cuda(),
                done=(torch.rand(TD_K * B, generator=g) < 0.2).to(torch.uint8).cuda(),
                sel=torch.randint(0, 5, (TD_K * B,), generator=g, dtype=torch.int32).cuda(),
                gamma_row=(0.5 + 0.5 * torch.rand(TD_K * B, generator=g)).cuda())


@pytest.mark.parametrize("opts", ["plain", "sel", "gamma_row", "sel+gamma_row"])
@pytest.mark.parametrize("B", [190, 256, 258])
def test_td_loss_opt_nets_equals_single_net_calls(B, opts):
    """evx_td_loss_opt_nets with deltas (0, 0.5, 10) against evx_td_loss_opt(nets = 1) on net k's block with
    its delta: dQ, td_abs and loss[k] by torch.equal; the extra workgroups clear the gradient buffer; equal
    deltas give evx_td_loss_opt bit for bit. Each Huber net has at least a tenth of its rows on either side
    of its delta (asserted on the reference's td_abs)."""
    _need_gpu()
    from evacx._lib import check, lib
    from evacx.qmlp import td_opts
    x = _td_inputs(B)
    sel = x["sel"] if "sel" in opts else None
    grow = x["gamma_row"] if "gamma_row" in opts else None
    L, K = lib(), TD_K
    ws = torch.zeros(int(L.evx_td_loss_ws_floats(B, K)), device="cuda")

    def nets_call(deltas):
        dQ_w, dQ = _padded(K * B * 5, torch.float32, 9.0)
        td_w, td = _padded(K * B, torch.float32, 9.0)
        loss_w, loss = _padded(K, torch.float32, 9.0)
        zero = torch.ones(5000, device="cuda")
        o = td_opts(sel=sel, huber_delta=float("nan"), gamma_row=grow)  # (opt->huber_delta is not read)
        check(L.evx_td_loss_opt_nets(x["Q"].data_ptr(), x["Qt"].data_ptr(), 5, x["a"].data_ptr(), x["r"].data_ptr(),
                                     x["done"].data_ptr(), 0.9, B, K, None, dQ.data_ptr(), loss.data_ptr(),
                                     td.data_ptr(), zero.data_ptr(), zero.numel(), ws.data_ptr(), ws.numel(),
                                     C.byref(o), (C.c_float * K)(*deltas), None), "td_loss_opt_nets")
        torch.cuda.synchronize()
        assert _pads_intact(dQ_w, K * B * 5, 9.0) and _pads_intact(td_w, K * B, 9.0) and _pads_intact(loss_w, K, 9.0)
        assert bool((zero == 0).all())
        return dQ.clone(), td.clone(), loss.clone()

    def opt_call(k0, nets, delta):
        rows = slice(k0 * B, (k0 + nets) * B)
        dQ, td = torch.zeros(nets * B * 5, device="cuda"), torch.zeros(nets * B, device="cuda")
        loss, w1 = torch.zeros(nets, device="cuda"), torch.zeros(int(L.evx_td_loss_ws_floats(B, nets)), device="cuda")
        o = td_opts(sel=None if sel is None else sel[rows], huber_delta=delta,
                    gamma_row=None if grow is None else grow[rows])
        check(L.evx_td_loss_opt(x["Q"][rows].data_ptr(), x["Qt"][rows].data_ptr(), 5, x["a"][rows].data_ptr(),
                                x["r"][rows].data_ptr(), x["done"][rows].data_ptr(), 0.9, B, nets, None, dQ.data_ptr(),
                                loss.data_ptr(), td.data_ptr(), None, 0, w1.data_ptr(), w1.numel(), C.byref(o), None),
              "td_loss_opt")
        torch.cuda.synchronize()
        return dQ, td, loss

    dQ, td, loss = nets_call(TD_DELTAS)
    for k, delta in enumerate(TD_DELTAS):
        rdQ, rtd, rloss = opt_call(k, 1, delta)
        assert torch.equal(dQ[k * B * 5:(k + 1) * B * 5], rdQ), k
        assert torch.equal(td[k * B:(k + 1) * B], rtd), k
        assert torch.equal(loss[k:k + 1], rloss), k
        if delta > 0:
            below = float((rtd <= delta).float().mean())
            print(f"B {B} {opts} net {k}: {below:.3f} of the rows within delta {delta}")
            assert 0.1 <= below <= 0.9, (k, below)
    for delta in (0.0, 0.5):  # equal deltas: the grouped evx_td_loss_opt
        a, b = nets_call([delta] * K), opt_call(0, K, delta)
        for u, v in zip(a, b):
            assert torch.equal(u, v), delta


# ------------------------------------------------------------------ c. the grouped Polyak update
def _polyak_state(seed=40):
    """A GroupedLearner of 3 nets whose targets differ from the online nets (operands packed)."""
    from evacx.qgroup import GroupedLearner
    grp = GroupedLearner(3, seed=seed)
    g = torch.Generator().manual_seed(4)
    grp.tflat.copy_(grp.flat + torch.randn(3, grp.npar, generator=g).cuda() * 0.01)
    grp.fast_t.repack()
    torch.cuda.synchronize()
    return grp


def test_polyak_pack3_g_equals_single_net_updates():
    """evx_qmlp_polyak_pack3_g with taus (0, 0.005, 1): net 0's target and nine operand buffers keep their
    bits; nets 1 and 2 equal evx_qmlp_polyak_pack3 of the single net (target and operands); net 2's target
    is its online net. The online nets and their operands are not written."""
    _need_gpu()
    taus = (0.0, 0.005, 1.0)
    a, b = _polyak_state(), _polyak_state()
    assert torch.equal(a.tflat, b.tflat) and not torch.equal(a.tflat, a.flat)
    before = dict(tflat=a.tflat.clone(), flat=a.flat.clone(), **{n: a.fast_t.bufs[n].clone() for n in pu.OPERANDS})
    online_ops = {n: a.fast.bufs[n].clone() for n in pu.OPERANDS}
    a.soft_update(taus)
    for k in (1, 2):
        b.fast_t.nets[k].polyak_step(b.flat[k], b.tflat[k], taus[k])
    torch.cuda.synchronize()
    assert torch.equal(a.tflat[0], before["tflat"][0])
    for n in pu.OPERANDS:
        assert torch.equal(a.fast_t.bufs[n][0], before[n][0]), n
        assert torch.equal(a.fast.bufs[n], online_ops[n]), n
    assert torch.equal(a.flat, before["flat"])
    for k in (1, 2):
        assert torch.equal(a.tflat[k], b.tflat[k]) and not torch.equal(a.tflat[k], before["tflat"][k]), k
        for n in pu.OPERANDS:
            assert torch.equal(a.fast_t.bufs[n][k], b.fast_t.bufs[n][k]), (k, n)
    assert torch.equal(a.tflat[2], a.flat[2]) and not torch.equal(a.tflat[1], a.flat[1])
    for n in pu.OPERANDS:  # tau 1: the target's operands are the online net's
        assert torch.equal(a.fast_t.bufs[n][2], a.fast.bufs[n][2]), n
    with pytest.raises(ValueError, match="taus must hold 3"):
        a.soft_update((0.1, 0.1))


# ------------------------------------------------------------------ d. the trainer
E, K, B, CAP, STEPS = 96, 3, 256, 1024, 12
HP = dict(lr=(1e-3, 3e-4, 1e-4), gamma=(0.99, 0.95, 0.9), epsilon=(1.0, 0.6, 0.3), epsilon_min=0.02,
          epsilon_decay=(0.9, 0.8, 0.95), target_every=(2, 3, 5))
OPTS = dict(double_q=True, loss=("mse", "huber", "huber"), huber_delta=(1.0, 0.5, 10.0), target_tau=(0.0, 0.01, 0.0),
            n_step=(1, 3, 2))
_RUNS = {}


def _run(key, cls=None, steps=STEPS, **over):
    """`steps` steps of a population (or of SlowPopulationOpts) with the actions, reward, done and losses
    of every step on the host: made once per key, shared by the tests below."""
    if key in _RUNS:
        return _RUNS[key]
    from evacx.population import PopulationTrainer
    kw = dict(HP)
    kw.update(over)
    tr = (cls or PopulationTrainer)(pu.small_layout(), E, members=K, seed=5, batch=B, replay_capacity=CAP, **kw)
    rec = dict(actions=[], reward=[], done=[], loss=[])
    for _ in range(steps):
        tr.step()
        torch.cuda.synchronize()
        rec["actions"].append(tr.actions.cpu().clone())
        rec["reward"].append(tr.env.reward.cpu().clone())
        rec["done"].append(tr.env.done.cpu().clone())
        rec["loss"].append(None if tr.last_loss is None else tr.last_loss.cpu().clone())
    tr.env.check_err()
    _RUNS[key] = (tr, rec)
    return _RUNS[key]


def _assert_equals_slow(pop, rp, slow, rs):
    assert pop.learn_steps == slow.learn_steps == STEPS - 1
    for t in range(STEPS):
        for name in ("actions", "reward", "done"):
            assert torch.equal(rp[name][t], rs[name][t]), (t, name)
        if rs["loss"][t] is None:
            assert rp["loss"][t] is None
            continue
        for k in range(K):
            a, b = rp["loss"][t][k].item(), rs["loss"][t][k].item()
            print(f"step {t} member {k}: loss {a!r} slow {b!r}")
            assert abs(a - b) <= 1e-6 * abs(b), (t, k, a, b)
    gl = pop.glearner
    for k, lr in enumerate(slow.learners):
        assert torch.equal(gl.flat[k], lr.online.flat), k
        assert torch.equal(gl.tflat[k], lr.target.flat), k
        assert torch.equal(gl.m[k], lr.m) and torch.equal(gl.v[k], lr.v), k
    assert gl.drop_stream == slow.drop_stream


def _assert_nlen(pop):
    torch.cuda.synchronize()
    nlen = pop.last_nlen
    assert nlen.dtype == torch.int32 and nlen.is_cuda and nlen.numel() == K * B
    for k in range(K):
        assert int(nlen[k * B:(k + 1) * B].max()) == pop.n_step[k], k
        assert int(nlen[k * B:(k + 1) * B].min()) >= 1


def test_trainer_with_every_option_equals_slow_population():
    """Double-Q for all, loss (mse, huber, huber) with deltas (1, 0.5, 10), target_tau (0, 0.01, 0), n_step
    (1, 3, 2): actions, reward and done equal SlowPopulationOpts at every step; online, target, m and v by
    torch.equal at the end; the losses to 1e-6 relative (tests/test_population_gpu.py's bar and reason)."""
    _need_gpu()
    pop, rp = _run("opts", **OPTS)
    slow, rs = _run("slow-opts", cls=po.SlowPopulationOpts, **OPTS)
    _assert_equals_slow(pop, rp, slow, rs)
    _assert_nlen(pop)
    gl = pop.glearner
    assert gl.last_sel is not None and gl.last_sel.numel() == K * B and int(gl.last_sel.max()) <= 4
    for k, lr in enumerate(slow.learners):
        assert torch.equal(gl.last_sel[k * B:(k + 1) * B], lr.last_sel[:B]), k
    # member 1 is soft: its target is neither its online net nor a hard copy's
    assert not torch.equal(gl.tflat[1], gl.flat[1])


def test_trainer_with_n_step_alone_equals_slow_population():
    _need_gpu()
    pop, rp = _run("nstep", n_step=OPTS["n_step"])
    slow, rs = _run("slow-nstep", cls=po.SlowPopulationOpts, n_step=OPTS["n_step"])
    _assert_equals_slow(pop, rp, slow, rs)
    _assert_nlen(pop)
    assert pop.glearner.last_sel is None


def _members_equal(a, b, k):
    return all(torch.equal(getattr(a.glearner, name)[k], getattr(b.glearner, name)[k])
               for name in ("flat", "tflat", "m", "v"))


def test_every_option_changes_its_members_and_only_them():
    """A run against the same run without one option. A member that had the option differs in its
    parameters (online, target, m or v) and in its last loss; a member whose options did not change keeps
    actions, parameters and losses bit for bit -- with member 1's target_tau alone changed these are
    members 0 and 2: the members are independent.

    Huber and target_tau are taken out of the full run. n-step and Double-Q are also put into the plain
    run, alone, and it is there that the parameters must differ: in the full run both n-step members are
    Huber members, and at this env's reward scale (|d| in the hundreds, deltas 0.5 and 10) their
    gradients are +-delta whatever the target's value is, so taking n-step or Double-Q out of the full run
    moves their losses and not their parameters (measured: no buffer of members 1 and 2 differs without
    n-step, every loss does). Out of the full run the losses of the changed members must differ and the
    others must not move."""
    _need_gpu()
    full, plain = _run("opts", **OPTS), _run("plain")
    N = full[0].N
    for key, base, over, changed, params in (
            ("no-huber", full, dict(OPTS, loss="mse"), (1, 2), True),
            ("no-tau", full, dict(OPTS, target_tau=0.0), (1,), True),
            ("no-nstep", full, dict(OPTS, n_step=1), (1, 2), False),
            ("no-dq", full, dict(OPTS, double_q=False), (0, 1, 2), False),
            ("nstep", plain, dict(n_step=OPTS["n_step"]), (1, 2), True),
            ("dq", plain, dict(double_q=True), (0, 1, 2), True)):
        (pop, ra), (oth, rb) = base, _run(key, **over)
        diff = {k: [name for name in ("flat", "tflat", "m", "v")
                    if not torch.equal(getattr(pop.glearner, name)[k], getattr(oth.glearner, name)[k])] for k in range(K)}
        loss_differs = [ra["loss"][-1][k].item() != rb["loss"][-1][k].item() for k in range(K)]
        print(f"{key}: buffers that differ per member {diff}, last loss differs {loss_differs}")
        for k in range(K):
            if k in changed:
                assert loss_differs[k], (key, k)
                assert diff[k] or not params, (key, k)
                continue
            assert not diff[k] and not loss_differs[k], (key, k, diff[k])
            for t in range(STEPS):
                assert torch.equal(ra["actions"][t][k * N:(k + 1) * N], rb["actions"][t][k * N:(k + 1) * N]), (key, t)
                assert (ra["loss"][t] is None) or ra["loss"][t][k].item() == rb["loss"][t][k].item(), (key, t, k)
        if key == "no-dq":  # the mse member's parameters do move
            assert diff[0], diff


# ------------------------------------------------------------------ e. defaults and the other entry points
def test_defaults_spelled_out_change_nothing():
    """Every new argument at its default: the launches, dropout stream numbers and bits of a trainer built
    without them -- actions at every step, all five flat buffers, both nets' operands, drop_stream; nothing
    is allocated for the options."""
    _need_gpu()
    a, ra = _run("plain")
    b, rb = _run("plain-spelled", double_q=False, loss="mse", huber_delta=1.0, target_tau=0.0, n_step=1)
    for t in range(STEPS):
        for name in ("actions", "reward", "done"):
            assert torch.equal(ra[name][t], rb[name][t]), (t, name)
        assert (ra["loss"][t] is None) == (rb["loss"][t] is None)
        if ra["loss"][t] is not None:
            assert torch.equal(ra["loss"][t], rb["loss"][t]), t
    for name in ("flat", "tflat", "gflat", "m", "v"):
        assert torch.equal(getattr(a.glearner, name), getattr(b.glearner, name)), name
    for name in pu.OPERANDS:
        assert torch.equal(a.glearner.fast.bufs[name], b.glearner.fast.bufs[name]), name
        assert torch.equal(a.glearner.fast_t.bufs[name], b.glearner.fast_t.bufs[name]), name
    assert a.glearner.drop_stream == b.glearner.drop_stream == STEPS + 2 * a.learn_steps
    assert b.last_nlen is None and "gamma_row" not in b.samp and b.glearner.last_sel is None
    assert "sel" not in b.glearner._ws


def _small_pop(**kw):
    from evacx.population import PopulationTrainer
    args = dict(members=3, seed=2, batch=64, replay_capacity=256, lr=1e-3, epsilon=(0.5, 0.2, 0.0), epsilon_decay=1.0,
                target_every=4)
    args.update(kw)
    return PopulationTrainer(pu.small_layout(), 24, **args)


def test_set_hparams_options_take_effect_at_the_next_step_only():
    """Two equal populations; one sets member 1's n_step to 2 and its target_tau to 0.5 after step 3. Every
    member is equal up to there; after the next step members 0 and 2 stay equal bit for bit, member 1's
    target has moved towards its online net, its chains reach 2 and its parameters differ. double_q, bad
    values and an n_step the ring cannot hold are refused."""
    _need_gpu()
    a, b = _small_pop(), _small_pop()
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.glearner.flat, b.glearner.flat) and torch.equal(a.glearner.tflat, b.glearner.tflat)
    b.set_hparams(1, n_step=2, target_tau=0.5)
    assert b.n_step == [1, 2, 1] and b.target_tau == [0.0, 0.5, 0.0] and a.n_step == [1, 1, 1]
    torch.cuda.synchronize()
    assert torch.equal(a.glearner.tflat, b.glearner.tflat) and b.last_nlen is None
    a.step()
    b.step()
    torch.cuda.synchronize()
    N, Bm = a.N, a.batch
    for k in (0, 2):
        assert _members_equal(a, b, k), k
        assert torch.equal(a.actions[k * N:(k + 1) * N], b.actions[k * N:(k + 1) * N]), k
    assert not torch.equal(a.glearner.tflat[1], b.glearner.tflat[1])
    assert not torch.equal(a.glearner.flat[1], b.glearner.flat[1])
    nlen = b.last_nlen.cpu()
    assert int(nlen[Bm:2 * Bm].max()) == 2 and bool((nlen[:Bm] == 1).all()) and bool((nlen[2 * Bm:] == 1).all())
    b.set_hparams(2, loss="huber", huber_delta=0.25)
    assert b.loss == ["mse", "mse", "huber"] and b.huber_delta[2] == 0.25
    for bad in (dict(double_q=True), dict(n_step=0), dict(n_step=9), dict(target_tau=1.5), dict(loss="l1"),
                dict(huber_delta=0.0)):
        with pytest.raises(ValueError):
            b.set_hparams(0, **bad)
    assert b.n_step == [1, 2, 1] and b.loss == ["mse", "mse", "huber"]


def test_member_learner_carries_the_options():
    _need_gpu()
    pop = _small_pop(double_q=True, loss=("mse", "huber", "huber"), huber_delta=(1.0, 0.5, 10.0),
                     target_tau=(0.0, 0.01, 1.0))
    for _ in range(3):
        pop.step()
    for k in range(3):
        lr = pop.member_learner(k)
        torch.cuda.synchronize()
        assert lr.double_q is True and lr.loss_kind == pop.loss[k] and lr.huber_delta == pop.huber_delta[k]
        assert lr.target_tau == pop.target_tau[k] and (lr.lr, lr.gamma) == (pop.lr[k], pop.gamma[k])
        assert torch.equal(lr.online.flat, pop.glearner.flat[k]) and torch.equal(lr.target.flat, pop.glearner.tflat[k])
    assert torch.equal(pop.glearner.tflat[2], pop.glearner.flat[2])  # tau 1: the target follows every step


def test_train_pop_runner_with_the_option_flags_writes_its_files(tmp_path, capsys):
    _need_gpu()
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(pu.__file__)), "..", "dqn-marl_amd"))
    from Louvre_Evacuation.runners import train_pop
    from Louvre_Evacuation.runners.evaluate_vec import load_learner
    cfg = tmp_path / "small.yaml"
    cfg.write_text("env:\n  width: 36\n  height: 30\n  fire_zones: [[18, 14]]\n  exit_location: [36, 15]\n"
                   "  num_people: 40\nagent:\n  gamma: 0.99\n  epsilon: 1.0\n  epsilon_min: 0.02\n"
                   "  epsilon_decay: 0.9995\n  learning_rate: 0.0001\n  batch_size: 32\n  target_update_freq: 20\n"
                   "  memory_size: 64\nsave_path: \"unused\"\n")
    out = tmp_path / "out"
    tr = train_pop.main(["--config", str(cfg), "--members", "2", "--envs", "16", "--steps", "6", "--log-every", "3",
                         "--lr", "1e-3,1e-4", "--batch", "16", "--out", str(out), "--double-q", "--loss", "mse,huber",
                         "--huber-delta", "0.5", "--target-tau", "0,0.01", "--n-step", "1,3"])
    assert tr.double_q is True and tr.loss == ["mse", "huber"] and tr.huber_delta == [0.5, 0.5]
    assert tr.target_tau == [0.0, 0.01] and tr.n_step == [1, 3]
    assert tr.replay.capacity >= 3 * tr.N and tr.last_nlen is not None
    text = capsys.readouterr().out
    assert "double-Q target" in text and "n_step [1, 3]" in text and "target tau [0.0, 0.01]" in text
    for k in range(2):
        rows = list(csv.reader(open(out / f"member{k}" / "training_log.csv")))
        assert rows[0] == train_pop.CSV_COLUMNS and [r[0] for r in rows[1:]] == ["3", "6"]
        lr = load_learner(str(out / f"member{k}" / "dqn_model.pth"), "cuda")
        torch.cuda.synchronize()
        assert torch.equal(lr.online.flat, tr.glearner.flat[k]), k
    assert os.path.exists(out / "population_summary.csv") and os.path.exists(out / "best_member.json")
    assert np.isfinite(tr.last_loss.cpu().numpy()).all()
