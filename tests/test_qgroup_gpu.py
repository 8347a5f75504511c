"""GPU parity of the grouped independent nets (evacx.qgroup, SURVEY §8f F3: one network per robot
as runners/train_double_dqn.py:35-56 trains them, and the QMIX mixer of runners/train_qmix.py:39-118).

* grouped learn == G separate evacx.qnet.Learner steps (same initial weights, same dropout
  keys), bit for bit: norms, clipped gradients, parameters, Adam state and every operand copy (the
  learn chain has no atomic sum: every reduction runs in a fixed order); the loss within 1e-6 (the
  two paths add a net's squared errors in different block sizes and orders: ulps);
* grouped act == the single-net act per robot (Q bit for bit, dropout keyed by the net's own
  batch rows) and epsilon draws keyed by the data row as the shared-net act;
* evx_qmix_loss (mixer forward, MSE, backward into every agent's dQ, mixer gradient) vs torch
  autograd of MixingNetwork (f32 tolerance: different summation order);
* GroupedQMix's learn steps vs torch fp32 autograd of the agents and MixingNetwork (loss,
  clipped gradients, agent and mixer parameters after Adam).
"""
import numpy as np
import pytest
import torch

import learn_util as lu

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _env_obs(E=96, steps=5, R=4, grid=48, people=300):
    from evacx.env import DeviceLayout, VecEnv
    from evacx.layout import build_tables, synthetic
    lay = DeviceLayout(build_tables(synthetic(grid, grid, R)), people)
    env = VecEnv(lay, E)
    env.seed([91 + i for i in range(E)])
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(steps):
        env.step(torch.randint(0, 5, (E * R,), device="cuda", dtype=torch.int32, generator=g))
    torch.cuda.synchronize()
    return lay, env


def _batch(env, G, B, g):
    obs = env.obs.view(-1, 8)
    n = obs.shape[0]
    s = obs[torch.randint(0, n, (G * B,), generator=g).cuda()].contiguous().view(-1)
    s2 = obs[torch.randint(0, n, (G * B,), generator=g).cuda()].contiguous().view(-1)
    a = torch.randint(0, 5, (G * B,), generator=g, dtype=torch.int32).cuda()
    r = (torch.randn(G * B, generator=g) * 30).cuda()
    d = (torch.rand(G * B, generator=g) < 0.2).to(torch.uint8).cuda()
    return s, s2, a, r, d


OPERANDS = ("w1b", "w1l", "b1c", "w2b", "w2l", "w2t", "w2tl", "w1o", "w1ol")  # MLPFast.buffer_sizes(x3)


@pytest.mark.parametrize("G,B", [(3, 256), (2, 190), (16, 1410), (2, 2050)])
def test_grouped_learn_equals_separate_learners(G, B):
    """evacx/qgroup.py's contract, bit for bit (torch.equal): norm, clipped gradients, parameters, m, v
    and every operand copy of both nets (online: repacked by the Adam launch; target: by sync_target)
    of a grouped step equal G separate Learner steps. (16, 1410): the 128-row fc1 beside the single
    net's 64 x 256 tiles; (2, 2050): qbwd3's 16-row band.

    The loss alone is not bit-equal, and is held to the bar it had (1e-6 relative): measured on an
    MI355X it differs by one or two f32 ulps in about a quarter of the (step, net) pairs of these
    cases. It is the one sum the two paths take in different orders: the grouped chain's
    td_loss_kernel adds a net's squared errors per 256-row block in an LDS tree and td_finish_kernel
    adds the blocks; the single net's TD step runs inside qbwd3_kernel, which adds them per 32 / 16 /
    64 / 128-row block in row order, and reduce2_kernel adds the blocks. Both are deterministic, dQ
    is the same expression in both, and nothing downstream reads the loss."""
    _need_gpu()
    from evacx.qgroup import GroupedLearner
    from evacx.qnet import Learner
    lay, env = _env_obs()
    grp = GroupedLearner(G, seed=40, lr=1e-3)
    sep = []
    for k in range(G):
        lr = Learner(kind="mlp", precision="f32", seed=40 + k, lr=1e-3)
        lr.seed = grp.seed  # the dropout hash seed; rows keyed k * B + i below
        sep.append(lr)
        assert torch.equal(lr.online.flat, grp.flat[k])
    g = torch.Generator().manual_seed(5)
    differ = []
    for it in range(3):
        s, s2, a, r, d = _batch(env, G, B, g)
        loss = grp.learn_obs(lay.c, s, a, r, d, s2, B).clone()
        for k, lr in enumerate(sep):
            rows = slice(k * B, (k + 1) * B)
            lk = lr.learn_obs(lay.c, s.view(-1, 8)[rows].contiguous().view(-1), a[rows].contiguous(),
                              r[rows].contiguous(), d[rows].contiguous(), s2.view(-1, 8)[rows].contiguous().view(-1),
                              B, drop_row0=k * B)
            torch.cuda.synchronize()
            assert abs(loss[k].item() - lk.item()) <= 1e-6 * abs(lk.item()), (it, k, loss[k].item(), lk.item())
            pairs = [("norm", grp.norm[k], lr.norm.reshape(-1)[0]), ("grads", grp.gflat[k], lr.grads.flat), ("params", grp.flat[k], lr.online.flat),
                     ("m", grp.m[k], lr.m), ("v", grp.v[k], lr.v)]
            pairs += [(name, grp.fast.bufs[name][k], getattr(lr.fast, name)) for name in OPERANDS]
            pairs += [("target " + name, grp.fast_t.bufs[name][k], getattr(lr.fast_t, name)) for name in OPERANDS]
            for name, x, y in pairs:
                assert x.shape == y.shape and x.dtype == y.dtype, (name, x.shape, y.shape)
                if not torch.equal(x, y):
                    n = int((x != y).sum())
                    worst = (x.double() - y.double()).abs().max().item()
                    print(f"G={G} B={B} step {it} net {k}: {name} differs in {n} of {x.numel()} elements, max {worst:.3e}")
                    differ.append((it, k, name, n, worst))
        if it == 1:
            grp.sync_target()
            for lr in sep:
                lr.sync_target()
    assert not differ, differ
    assert len({round(float(x), 3) for x in loss}) == G  # the nets really differ


@pytest.mark.parametrize("eps", [0.0, 1.0])
def test_grouped_act_equals_single_net_act(eps):
    _need_gpu()
    from evacx.qgroup import GroupedLearner
    from evacx.qmlp import NACT
    R = 4
    lay, env = _env_obs(E=300, R=R)
    E = env.E
    grp = GroupedLearner(R, seed=8)
    q = torch.full((E * R, NACT), 7.0, device="cuda")
    act = torch.full((E * R,), -1, dtype=torch.int32, device="cuda")
    grp.act(lay.c, env.obs, E, actions=act, q=q, epsilon=eps, act_seed=9, act_offset=33, drop_stream=12)
    obs = env.obs.view(E, R, 8)
    for k in range(R):
        ok = obs[:, k].contiguous().view(-1)
        qk = torch.empty(E, NACT, device="cuda")
        ak = torch.empty(E, dtype=torch.int32, device="cuda")
        grp.fast.nets[k].act(lay.c, ok, E, drop=(grp.seed, 12, 0.2, None, k * E), q=qk, actions=ak)
        torch.cuda.synchronize()
        assert torch.equal(q.view(E, R, NACT)[:, k], qk), k
        if eps == 0.0:
            assert torch.equal(act.view(E, R)[:, k], ak), k
    if eps == 1.0:  # every action drawn: keyed by the data row (env * R + robot), as the shared-net act
        ref = torch.empty(E * R, dtype=torch.int32, device="cuda")
        grp.fast.nets[0].act(lay.c, env.obs, E * R, drop=(grp.seed, 12, 0.2), actions=ref, epsilon=1.0, act_seed=9,
                             act_offset=33)
        torch.cuda.synchronize()
        assert torch.equal(act, ref)


@pytest.mark.parametrize("eps", [0.0, 1.0])
@pytest.mark.parametrize("R,n", [(16, 2), (16, 62), (16, 66), (32, 2), (32, 62), (32, 66)])
def test_grouped_act_at_robot_counts(R, n, eps):
    """test_grouped_act_equals_single_net_act at the robot counts of BASELINE cfg3 (16) and cfg5 (32),
    n rows per net: one row pair, one 64-row tile short of a pair, one tile plus a pair. Q equals the
    single-net act of every robot bit for bit (dropout keyed by the net's own rows); the actions equal
    the single-net act's at eps 0 and oracle.epsilon_greedy of the kernel's Q, keyed by the data row
    (env * R + robot), at eps 1."""
    _need_gpu()
    from evacx.qgroup import GroupedLearner
    from evacx.qmlp import NACT
    from oracle import oracle as orc
    lay, env = _env_obs(E=n, R=R)
    E = env.E
    assert E == n
    grp = GroupedLearner(R, seed=8)
    q = torch.full((E * R, NACT), 7.0, device="cuda")
    act = torch.full((E * R,), -1, dtype=torch.int32, device="cuda")
    grp.act(lay.c, env.obs, E, actions=act, q=q, epsilon=eps, act_seed=9, act_offset=33, drop_stream=12)
    torch.cuda.synchronize()
    obs = env.obs.view(E, R, 8)
    seen = set()
    for k in range(R):
        ok = obs[:, k].contiguous().view(-1)
        qk = torch.empty(E, NACT, device="cuda")
        ak = torch.empty(E, dtype=torch.int32, device="cuda")
        grp.fast.nets[k].act(lay.c, ok, E, drop=(grp.seed, 12, 0.2, None, k * E), q=qk, actions=ak)
        torch.cuda.synchronize()
        assert torch.equal(q.view(E, R, NACT)[:, k], qk), k
        if eps == 0.0:
            assert torch.equal(act.view(E, R)[:, k], ak), k
        seen.add(tuple(qk[0].tolist()))
    assert len(seen) == R  # the nets really differ
    if eps == 1.0:
        assert np.array_equal(act.cpu().numpy(), orc.epsilon_greedy(q.cpu().numpy(), 1.0, 9, 33))


def test_qmix_kernel_matches_torch_autograd():
    _need_gpu()
    from evacx.qmix import MixingNetwork
    from evacx._lib import lib
    n, B, A = 3, 700, 5
    torch.manual_seed(2)
    mix, mix_t = MixingNetwork(n).cuda(), MixingNetwork(n).cuda()
    with torch.no_grad():
        mix.fc1_bias.normal_()
        mix.fc2_bias.normal_()
        mix.fc1_weight[0, 3] = 0.0  # sign(0) = 0 in torch.abs' gradient
    Q = torch.randn(n, B, A, device="cuda") * 5
    Qt = torch.randn(n, B, A, device="cuda") * 5
    act = torch.randint(0, A, (n, B), device="cuda", dtype=torch.int32)
    rew = torch.randn(B, device="cuda") * 10
    done = (torch.rand(B, device="cuda") < 0.3).to(torch.uint8)
    flat = torch.cat([p.detach().reshape(-1) for p in mix.state_dict().values()])
    flat_t = torch.cat([p.detach().reshape(-1) for p in mix_t.state_dict().values()])
    nm = int(lib().evx_qmix_nparams(n))
    assert nm == flat.numel()
    dQ = torch.full((n, B, A), 5.0, device="cuda")
    grad = torch.empty(nm, device="cuda")
    loss = torch.empty(1, device="cuda")
    part = torch.empty(int(lib().evx_qmix_part_floats(B, n)), device="cuda")
    zero = torch.ones(1000, device="cuda")
    rc = lib().evx_qmix_loss(Q.data_ptr(), Qt.data_ptr(), A, act.data_ptr(), rew.data_ptr(), done.data_ptr(), 0.99, B,
                             n, flat.data_ptr(), flat_t.data_ptr(), dQ.data_ptr(), grad.data_ptr(), loss.data_ptr(),
                             part.data_ptr(), zero.data_ptr(), zero.numel(), None)
    assert rc == 0
    q = Q.gather(2, act.long().unsqueeze(2)).squeeze(2).t().contiguous().requires_grad_(True)  # [B][n]
    with torch.no_grad():
        y = rew + 0.99 * mix_t(Qt.max(2)[0].t()) * (~done.bool()).float()
    ref = torch.nn.functional.mse_loss(mix(q), y)
    mix.zero_grad()
    ref.backward()
    torch.cuda.synchronize()
    assert torch.count_nonzero(zero) == 0
    torch.testing.assert_close(loss[0], ref.detach(), rtol=1e-5, atol=1e-6)
    gref = torch.cat([p.grad.reshape(-1) for p in mix.parameters()])
    torch.testing.assert_close(grad, gref, rtol=1e-4, atol=1e-5 * gref.abs().max().item())
    assert grad[3].item() == 0.0
    dref = torch.zeros(n, B, A, device="cuda")
    dref.scatter_(2, act.long().unsqueeze(2), q.grad.t().unsqueeze(2))
    torch.testing.assert_close(dQ, dref, rtol=1e-4, atol=1e-6 * dref.abs().max().item())


def test_grouped_qmix_step_matches_torch_autograd():
    """Two QMIX learn steps (runners/train_qmix.py:78-113) from the same state: GroupedQMix
    (grouped x3 kernels + evx_qmix_loss + per-agent clip/Adam + mixer clip/Adam) vs torch fp32
    autograd of the agents' fc stacks and MixingNetwork on the expanded observations, dropout off
    on both sides (p = 0): loss, clipped agent gradients, agent parameters, mixer parameters."""
    _need_gpu()
    import torch.nn.functional as F
    from evacx.qgroup import GroupedLearner, GroupedQMix
    from evacx.qmix import MixingNetwork
    from evacx.qmlp import K1
    n, B = 2, 128
    lay, env = _env_obs(R=2)
    grp = GroupedLearner(n, seed=60, lr=1e-3)
    grp.drop_p = 0.0
    torch.manual_seed(3)
    mixing, target_mixing = MixingNetwork(n).cuda(), MixingNetwork(n).cuda()
    target_mixing.load_state_dict(mixing.state_dict())
    qm = GroupedQMix(grp, mixing=mixing)
    agents = [{k: torch.nn.Parameter(v.clone()) for k, v in grp.online[j].state_dict().items()} for j in range(n)]
    targets = [{k: v.clone() for k, v in grp.target[j].state_dict().items()} for j in range(n)]
    opts = [torch.optim.Adam(p.values(), lr=1e-3) for p in agents]
    mopt = torch.optim.Adam(mixing.parameters(), lr=1e-3)

    def fc(sd, X):
        h = F.relu(F.linear(X, sd["fc1.weight"], sd["fc1.bias"]))
        h = F.relu(F.linear(h, sd["fc2.weight"], sd["fc2.bias"]))
        return F.linear(h, sd["fc3.weight"], sd["fc3.bias"])
    g = torch.Generator().manual_seed(4)
    for it in range(2):
        s, s2, a, _, _ = _batch(env, n, B, g)
        r = (torch.randn(B, generator=g) * 30).cuda()
        d = (torch.rand(B, generator=g) < 0.2).to(torch.uint8).cuda()
        loss = qm(lay.c, s, a, r, d, s2, B)
        X = env.expand_obs(torch.float32, s).reshape(n, B, K1)
        X2 = env.expand_obs(torch.float32, s2).reshape(n, B, K1)
        av = a.view(n, B).long()
        q = torch.stack([fc(agents[j], X[j]).gather(1, av[j].unsqueeze(1)).squeeze(1) for j in range(n)], 1)
        with torch.no_grad():
            qt = torch.stack([fc(targets[j], X2[j]).max(1)[0] for j in range(n)], 1)
            y = r + 0.99 * target_mixing(qt) * (~d.bool())
        ref = F.mse_loss(mixing(q), y)
        for o in opts + [mopt]:
            o.zero_grad()
        ref.backward()
        norms = [torch.nn.utils.clip_grad_norm_(p.values(), 1.0) for p in agents]
        mnorm = torch.nn.utils.clip_grad_norm_(mixing.parameters(), 1.0)
        grads = [torch.cat([p.grad.reshape(-1) for p in ag.values()]) for ag in agents]
        for o in opts + [mopt]:
            o.step()
        torch.cuda.synchronize()
        assert abs(loss.item() - ref.item()) <= 2e-4 * abs(ref.item()) + 1e-5, (it, loss.item(), ref.item())
        for j in range(n):
            assert abs(grp.norm[j].item() - norms[j].item()) <= 2e-4 * norms[j].item() + 1e-6, (it, j)
            # x3 products (~2^-16 relative) under cancellation: a few of 5e5 elements beyond rtol 2e-3
            gs = grads[j].abs().max().item()
            bad = (grp.gflat[j] - grads[j]).abs() > 2e-3 * grads[j].abs() + 1e-5 * gs
            assert bad.float().mean().item() <= 1e-4, (it, j, int(bad.sum()))
            assert (grp.gflat[j] - grads[j]).abs().max().item() <= 1e-3 * gs, (it, j)
            pref = torch.cat([p.detach().reshape(-1) for p in agents[j].values()])
            diff = (grp.flat[j] - pref).abs()
            assert (diff > 1e-5).float().mean().item() <= 1e-3 and diff.max().item() <= 2e-3, (it, j)
        assert abs(qm.mix_norm.item() - mnorm.item()) <= 2e-4 * mnorm.item() + 1e-6
        mref = torch.cat([p.detach().reshape(-1) for p in mixing.state_dict().values()])
        torch.testing.assert_close(qm.mix, mref, rtol=1e-4, atol=1e-5)


def test_vec_trainer_per_robot_nets():
    """VecTrainer(nets="per_robot"): robot r of every env acts through net r (== the grouped act
    on the same observations and weights), every net learns from its own robot's transitions
    (the per-agent sampler) and moves; the shared-net parameters are untouched by construction."""
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    from evacx.trainer import VecTrainer
    R, E = 4, 64
    lay = DeviceLayout(build_tables(synthetic(48, 48, R)), 300)
    tr = VecTrainer(lay, E, batch=8 * R * 2, replay_capacity=1 << 12, nets="per_robot", epsilon=0.3, learner_seed=3)
    p0 = tr.glearner.flat.clone()
    for _ in range(6):
        tr.step()
    tr.sync()
    torch.cuda.synchronize()
    assert tr.last_loss is not None and tr.last_loss.shape == (R,) and torch.isfinite(tr.last_loss).all()
    moved = (tr.glearner.flat != p0).any(dim=1)
    assert bool(moved.all())
    # the next act == a grouped act with the trainer's draws
    a_ref = torch.empty(E * R, dtype=torch.int32, device="cuda")
    off = tr.t * tr.n_world + tr.agent0
    stream = 0x40000000 + tr.glearner._act_calls + 1
    tr.glearner.act(lay.c, tr.env.obs, E, actions=a_ref, epsilon=float(tr.epsilon), act_seed=tr.act_seed,
                    act_offset=off, drop_stream=stream)
    a = tr.act()
    torch.cuda.synchronize()
    assert torch.equal(a, a_ref)


def test_vec_trainer_qmix_nets():
    """VecTrainer(nets="qmix"): the robots of an env as the agents of runners/train_qmix.py --
    joint samples, GroupedQMix learn steps (mixer kernel), every agent and the mixer move."""
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    from evacx.trainer import VecTrainer
    R, E = 4, 64
    lay = DeviceLayout(build_tables(synthetic(48, 48, R)), 300)
    tr = VecTrainer(lay, E, batch=8 * R * 2, replay_capacity=1 << 12, nets="qmix", epsilon=0.3, learner_seed=5,
                    target_every=3)
    p0, m0 = tr.glearner.flat.clone(), tr.qmix.mix.clone()
    for _ in range(8):
        tr.step()
    tr.sync()
    torch.cuda.synchronize()
    assert tr.last_loss is not None and torch.isfinite(tr.last_loss).all()
    assert bool((tr.glearner.flat != p0).any(dim=1).all()) and not torch.equal(tr.qmix.mix, m0)
    assert torch.equal(tr.qmix.mix_t, tr.qmix.mix) or tr.learn_steps % 3 != 0


# ------------------------------------------------------------------ evx_qmix_loss against float64
GUARD = 8  # floats behind every output that must keep their sentinel


def _mixer_inputs(n, B, A, seed):
    """Inputs of one evx_qmix_loss call: Q / Qt [n][B][A], act [n][B], rew / done [B], both mixers
    flat in state_dict order (biases drawn too: MixingNetwork starts them at zero)."""
    g = torch.Generator().manual_seed(seed)
    c = lu.SimpleNamespace(n=n, B=B, A=A)
    c.Q = (torch.randn(n, B, A, generator=g) * 5).cuda()
    c.Qt = (torch.randn(n, B, A, generator=g) * 5).cuda()
    c.act = torch.randint(0, A, (n, B), generator=g, dtype=torch.int32).cuda()
    c.rew = (torch.randn(B, generator=g) * 10).cuda()
    c.done = (torch.rand(B, generator=g) < 0.3).to(torch.uint8).cuda()
    nm = n * 32 + 32 + 32 + 1
    c.mix = torch.randn(nm, generator=g).cuda()
    c.mix_t = torch.randn(nm, generator=g).cuda()
    return c


def _mixer_run(c, nzero=1000, zero_null=False):
    """evx_qmix_loss on c. Outputs pre-filled with sentinels (dQ: 5, the rest NaN) and followed by
    GUARD floats; the zero buffer (nzero + GUARD floats) pre-filled with ones."""
    from evacx._lib import lib
    L = lib()
    n, B, A = c.n, c.B, c.A
    nm = int(L.evx_qmix_nparams(n))
    assert nm == c.mix.numel()
    npart = int(L.evx_qmix_part_floats(B, n))
    o = lu.SimpleNamespace()
    o.dQ = torch.full((n * B * A + GUARD,), 5.0, device="cuda")
    o.grad = torch.full((nm + GUARD,), float("nan"), device="cuda")
    o.loss = torch.full((1 + GUARD,), float("nan"), device="cuda")
    o.part = torch.full((npart + GUARD,), float("nan"), device="cuda")
    o.zero = torch.ones(nzero + GUARD, device="cuda")
    o.rc = L.evx_qmix_loss(c.Q.data_ptr(), c.Qt.data_ptr(), A, c.act.data_ptr(), c.rew.data_ptr(), c.done.data_ptr(),
                           0.99, B, n, c.mix.data_ptr(), c.mix_t.data_ptr(), o.dQ.data_ptr(), o.grad.data_ptr(),
                           o.loss.data_ptr(), o.part.data_ptr(), None if zero_null else o.zero.data_ptr(),
                           0 if zero_null else nzero, None)
    torch.cuda.synchronize()
    assert o.rc == 0, L.evx_qmix_last_error()
    # nothing behind any output, the cleared span exactly
    assert bool((o.dQ[n * B * A:] == 5.0).all()) and bool(torch.isnan(o.grad[nm:]).all())
    assert bool(torch.isnan(o.loss[1:]).all()) and bool(torch.isnan(o.part[npart:]).all())
    assert bool((o.zero[nzero:] == 1.0).all()), "the clear wrote behind nzero floats"
    if zero_null:
        assert bool((o.zero == 1.0).all())
    else:
        assert torch.count_nonzero(o.zero[:nzero]) == 0, "the clear left floats uncleared"
    o.dQ, o.grad, o.loss = o.dQ[:n * B * A].view(n, B, A), o.grad[:nm], o.loss[0]
    return o


def _mixer_reference(c, dtype):
    """MixingNetwork (evacx/qmix.py) in `dtype` with autograd on c: (loss, mixer gradient flat in
    state_dict order, dQ [n][B][A] scattered at the taken actions, 0 elsewhere)."""
    from evacx.qmix import MixingNetwork
    n, B, A = c.n, c.B, c.A

    def net(flat):
        m = MixingNetwork(n).to("cuda", dtype)
        sd = lu.mixer_dict(flat, n)
        m.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
        return m
    mix, mix_t = net(c.mix), net(c.mix_t)
    ai = c.act.long().unsqueeze(2)
    q = c.Q.to(dtype).gather(2, ai).squeeze(2).t().contiguous().requires_grad_(True)  # [B][n]
    with torch.no_grad():
        y = c.rew.to(dtype) + 0.99 * mix_t(c.Qt.to(dtype).max(2)[0].t()) * (~c.done.bool()).to(dtype)
    loss = torch.nn.functional.mse_loss(mix(q), y)
    loss.backward()
    grad = torch.cat([p.grad.reshape(-1) for p in mix.parameters()])
    dQ = torch.zeros(n, B, A, device="cuda", dtype=dtype)
    dQ.scatter_(2, ai, q.grad.t().unsqueeze(2))
    return loss.detach(), grad, dQ


# the bars of test_qmix_kernel_matches_torch_autograd (set at n = 3), as (rtol, atol in max |ref|)
MIX_BARS = {"loss": (1e-5, 0.0), "grad": (1e-4, 1e-5), "dQ": (1e-4, 1e-6)}


def _mixer_errors(got, ref64):
    """The worst error of (loss, grad, dQ) against the float64 reference in units of MIX_BARS: <= 1
    passes torch.testing.assert_close at those bars (loss: atol 1e-6 as that test)."""
    out = {}
    for name, x, r in zip(("loss", "grad", "dQ"), got, ref64):
        rtol, atol = MIX_BARS[name]
        a = atol * r.abs().max().item() + (1e-6 if name == "loss" else 0.0)
        e = (x.double() - r).abs()
        out[name] = (e / (rtol * r.abs() + a + 1e-300)).max().item()
    return out


def _mixer_check(c, o, what, scale=1.0):
    """o against float64 at scale x MIX_BARS, the float32 torch evaluation's own error next to it;
    dQ exactly 0 off the taken actions."""
    ref64 = _mixer_reference(c, torch.float64)
    dev = _mixer_errors((o.loss, o.grad, o.dQ), ref64)
    f32 = _mixer_errors(_mixer_reference(c, torch.float32), ref64)
    print(f"{what}: loss {o.loss.item():.9g} ref {ref64[0].item():.9g}; error / bar: kernel " +
          ", ".join(f"{k} {v:.3f}" for k, v in dev.items()) + "; float32 torch " +
          ", ".join(f"{k} {v:.3f}" for k, v in f32.items()))
    assert torch.isfinite(o.loss) and torch.isfinite(o.grad).all() and torch.isfinite(o.dQ).all(), what
    taken = torch.zeros(c.n, c.B, c.A, dtype=torch.bool, device="cuda").scatter_(2, c.act.long().unsqueeze(2), True)
    assert bool((o.dQ[~taken] == 0).all()), f"{what}: dQ off the taken actions"
    for k, v in dev.items():
        assert v <= scale, f"{what}: {k} error {v:.3f} x its bar (float32 torch: {f32[k]:.3f})"
    return ref64


# n, B, A: every n of {1, 2, 5, 16}, every B of {1, 255, 256, 257, 700} (either side of a 256-row
# workgroup), every A of {1, 5, 64}; n = 16 at B = 257 and B = 700
MIX_CASES = [(1, 1, 1), (1, 256, 5), (2, 255, 5), (2, 257, 1), (2, 700, 64), (5, 256, 64), (5, 700, 5),
             (16, 1, 64), (16, 257, 5), (16, 700, 5)]


@pytest.mark.parametrize("n,B,A", MIX_CASES, ids=[f"n{n}-B{b}-A{a}" for n, b, a in MIX_CASES])
def test_qmix_kernel_matches_float64(n, B, A):
    """evx_qmix_loss against MixingNetwork in float64 with autograd: the loss (rtol 1e-5), the raw
    mixer gradient in state_dict order (rtol 1e-4, atol 1e-5 max |ref|) and dQ (rtol 1e-4, atol 1e-6
    max |ref|; exactly 0 off the taken actions, over a sentinel) -- the bars the n = 3 test set, which
    hold at every case here, n = 16 included. At A = 1 the only action is the maximum and the taken one.
    Two runs give bit-equal outputs.

    Measured on an MI355X at n = 16, worst error against float64 in units of those bars, the kernel
    next to a plain float32 torch evaluation of the same formula (the test prints both at every case):
      B = 257: kernel loss 0.026, gradient 0.005, dQ 0.006; float32 torch 0.014, 0.003, 0.006
      B = 700: kernel loss 0.018, gradient 0.002, dQ 0.007; float32 torch 0.004, 0.004, 0.006
    So the n = 3 bars hold at n = 16 with a margin of 38 or more and stay as they are. Four times the
    float32 evaluation's own error would be a bar of 1.6e-7 relative on the loss at B = 700 -- under two
    ulps of an f32 loss of 2.3e6, where torch's pairwise sum happened to land within one; the kernel's
    row-order sum is at 1.8e-7. That figure is a rounding, not a bar, and none was derived from it."""
    _need_gpu()
    c = _mixer_inputs(n, B, A, 100 * n + B + A)
    o = _mixer_run(c)
    _mixer_check(c, o, f"n={n} B={B} A={A}")
    o2 = _mixer_run(c)
    for name in ("loss", "grad", "dQ"):
        assert torch.equal(getattr(o, name), getattr(o2, name)), f"{name} differs between two runs"


def test_qmix_kernel_edges():
    """Each edge with its expected result from the formula q_tot = relu(q |W1| + b1) |W2| + b2,
    y = r + gamma q_tot'(max Qt) (1 - done), loss = mean((q_tot - y)^2)."""
    _need_gpu()
    n, B, A = 5, 257, 5
    nm = n * 32 + 65
    # a zero in fc1_weight and one in fc2_weight: torch.abs' gradient is sign(0) = 0 there; hidden unit
    # 7's |W2| = 0 also stops every gradient through it (column 7 of fc1_weight, fc1_bias[7])
    c = _mixer_inputs(n, B, A, 1)
    c.mix[2 * 32 + 3] = 0.0
    c.mix[n * 32 + 32 + 7] = 0.0
    o = _mixer_run(c)
    _mixer_check(c, o, "zero weights")
    assert o.grad[2 * 32 + 3].item() == 0.0 and o.grad[n * 32 + 32 + 7].item() == 0.0
    assert bool((o.grad[:n * 32].view(n, 32)[:, 7] == 0).all()) and o.grad[n * 32 + 7].item() == 0.0
    # Qt rows with tied maxima: the maximum is a value, whichever index holds it
    c = _mixer_inputs(n, B, A, 2)
    top = c.Qt.max(2)[0] + 1.0
    c.Qt[:, ::2, 1] = top[:, ::2]
    c.Qt[:, ::2, 3] = top[:, ::2]
    c.Qt[:, 1::4, :] = top[:, 1::4].unsqueeze(2)  # ... and rows that are one value throughout
    o_tie = _mixer_run(c)
    _mixer_check(c, o_tie, "tied maxima")
    # every row done: y = r, whatever the target mixer holds -- bit for bit
    c = _mixer_inputs(n, B, A, 3)
    c.done.fill_(1)
    o = _mixer_run(c)
    ref = _mixer_check(c, o, "all done")
    q = c.Q.double().gather(2, c.act.long().unsqueeze(2)).squeeze(2).t()
    want = ((lu.mixer64(lu.mixer_dict(c.mix, n), q) - c.rew.double()) ** 2).mean()
    assert abs(ref[0].item() - want.item()) <= 1e-12 * want.item()
    c.mix_t = torch.randn(nm, generator=torch.Generator().manual_seed(33)).cuda() * 100
    o2 = _mixer_run(c)
    for name in ("loss", "grad", "dQ"):
        assert torch.equal(getattr(o, name), getattr(o2, name)), f"all done: {name} depends on the target mixer"
    # biases so negative that the hidden layer is dead: q_tot = b2; every mixer gradient but fc2_bias'
    # is exactly 0, dQ is exactly 0, d loss / d b2 = mean(2 (b2 - y))
    c = _mixer_inputs(n, B, A, 4)
    c.mix[n * 32:n * 32 + 32] = -1e6
    o = _mixer_run(c)
    ref = _mixer_check(c, o, "dead hidden layer")
    assert torch.count_nonzero(o.grad[:nm - 1]) == 0 and torch.count_nonzero(o.dQ) == 0
    assert torch.count_nonzero(ref[1][:nm - 1]) == 0 and torch.count_nonzero(ref[2]) == 0
    assert o.grad[nm - 1].item() != 0.0
    # B = 0: returns 0 and writes nothing
    from evacx._lib import lib
    dQ = torch.full((64,), 5.0, device="cuda")
    out = torch.full((nm + 1 + 64,), float("nan"), device="cuda")
    zero = torch.ones(64, device="cuda")
    rc = lib().evx_qmix_loss(c.Q.data_ptr(), c.Qt.data_ptr(), A, c.act.data_ptr(), c.rew.data_ptr(), c.done.data_ptr(),
                             0.99, 0, n, c.mix.data_ptr(), c.mix_t.data_ptr(), dQ.data_ptr(), out.data_ptr(),
                             out[nm:].data_ptr(), out[nm + 1:].data_ptr(), zero.data_ptr(), 64, None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((dQ == 5.0).all()) and bool(torch.isnan(out).all()) and bool((zero == 1.0).all())


@pytest.mark.parametrize("nzero", [1, 512 * 256 * 16, 512 * 256 * 16 + 5], ids=["1", "cap", "cap+5"])
def test_qmix_kernel_clears_the_gradient_buffer(nzero):
    """The clear of zero[0, nzero): one float; 512 workgroups x 256 threads x 16 floats, the most the
    capped clear covers at 16 floats per thread; five more (each thread strides past the cap). All
    cleared, the 8 floats behind untouched (checked by _mixer_run), and zero = NULL gives the same
    outputs bit for bit and clears nothing."""
    _need_gpu()
    c = _mixer_inputs(2, 257, 5, 50)
    o = _mixer_run(c, nzero=nzero)
    o_null = _mixer_run(c, nzero=nzero if nzero == 1 else 16, zero_null=True)
    for name in ("loss", "grad", "dQ"):
        assert torch.equal(getattr(o, name), getattr(o_null, name)), name


def test_grouped_qmix_step_at_16_agents_matches_float64():
    """test_grouped_qmix_step_matches_torch_autograd at n = 16 agents and B = 1410 rows each (the
    128-row fc1 under the mixer), dropout on: two GroupedQMix steps, sync_targets() between, against
    the agents (tests/learn_util.py: float64, the device's own gates, the restated keep masks), both
    mixers and the MSE in float64 under one autograd backward -- each agent's output gradient is the
    mixer's dQ -- then clip_grad_norm_(1.0) + Adam per agent and for the mixer. The bars of that test:
    loss rtol 2e-4 (+1e-5); per-agent norm rtol 2e-4 (+1e-6); clipped gradients: at most 1e-4 of the
    elements beyond rtol 2e-3 + 1e-5 max |grad|, none beyond 1e-3 max |grad|; parameters: at most 1e-3
    of the elements beyond 1e-5, none beyond 2e-3; mixer norm rtol 2e-4 (+1e-6), mixer parameters rtol
    1e-4, atol 1e-5."""
    _need_gpu()
    from evacx.qgroup import GroupedLearner, GroupedQMix, group_plan
    from evacx.qmix import MixingNetwork
    n, B = 16, 1410
    assert group_plan(B, n).fc1_rows == 128, "this case no longer runs the 128-row fc1"
    lay, env = lu.small_env(4096)
    grp = GroupedLearner(n, seed=60, lr=1e-3)
    for j in range(n):
        grp.target[j].init_like_torch(1060 + j)
    grp.fast_t.repack()
    torch.manual_seed(3)
    mixing = MixingNetwork(n)
    with torch.no_grad():
        mixing.fc1_bias.normal_()
        mixing.fc2_bias.normal_()
    qm = GroupedQMix(grp, mixing=mixing.cuda())
    qm.mix_t.copy_(torch.randn(qm.nmix))  # a target mixer of its own
    gen = torch.Generator().manual_seed(4)
    for it in range(2):
        gb = lu.grouped_batch(env, n, B, gen)
        r = (torch.randn(B, generator=gen) * 30).cuda()
        d = (torch.rand(B, generator=gen) < 0.2).to(torch.uint8).cuda()
        dev, ref = lu.qmix_step_and_references(qm, lay, env, gb, r, d)
        print(f"step {it}: loss {dev.loss:.9g} ref {ref.loss:.9g}; mixer norm {dev.mix_norm:.9g} ref {ref.mix_norm:.9g}")
        assert abs(dev.loss - ref.loss) <= 2e-4 * abs(ref.loss) + 1e-5, (it, dev.loss, ref.loss)
        norms = set()
        for j, (dj, rj) in enumerate(zip(dev.agents, ref.agents)):
            gd = torch.cat([t.reshape(-1) for t in dj.grads.values()]).double()
            gr = torch.cat([t.reshape(-1) for t in rj.grads.values()])
            gs = gr.abs().max().item()
            err = (gd - gr).abs()
            bad = (err > 2e-3 * gr.abs() + 1e-5 * gs).double().mean().item()
            pd = torch.cat([t.reshape(-1) for t in dj.params.values()]).double()
            diff = (pd - torch.cat([t.reshape(-1) for t in rj.params.values()])).abs()
            print(f"step {it} agent {j}: norm {dj.norm:.9g} ref {rj.norm:.9g}; grads beyond the bar {bad:.2e}, max err "
                  f"{err.max().item():.3e} of max |grad| {gs:.3e}; params beyond 1e-5 "
                  f"{(diff > 1e-5).double().mean().item():.2e}, max {diff.max().item():.3e}")
            assert abs(dj.norm - rj.norm) <= 2e-4 * rj.norm + 1e-6, (it, j, dj.norm, rj.norm)
            assert bad <= 1e-4 and err.max().item() <= 1e-3 * gs, (it, j, bad, err.max().item(), gs)
            assert (diff > 1e-5).double().mean().item() <= 1e-3 and diff.max().item() <= 2e-3, (it, j)
            norms.add(dj.norm)
        assert len(norms) == n  # the agents really differ
        assert abs(dev.mix_norm - ref.mix_norm) <= 2e-4 * ref.mix_norm + 1e-6, (it, dev.mix_norm, ref.mix_norm)
        torch.testing.assert_close(dev.mix.double(), ref.mix, rtol=1e-4, atol=1e-5)
        if it == 0:
            qm.sync_targets()
