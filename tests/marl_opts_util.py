"""Helpers of the per-robot / QMIX learner-option tests: a numpy restatement of
evx_replay_sample_nstep_agents and the ring fixture it is checked on. The restatement is not the
code under test: the draws are replay_util.RingModel's sample_agents / sample_joint (the oracle's
keyed permutation), the chain is test_nstep_cpu.np_nstep (include/evacx.h's loop in np.float32
scalars)."""
import numpy as np

from replay_util import OBS_WORDS, RingModel
from test_nstep_cpu import np_nstep

CAP = 96
NETS = (2, 4)
ENVS = 2  # envs per push: the chains' stride is ENVS * nets rows
NSTEPS = (1, 2, 3, 5)
STATES = ("part", "full", "wrapped")
SEED, OFFSET = 77, 1000


def stride_of(nets):
    return ENVS * nets


def pushes_of(nets, state):
    """Pushes of ENVS * nets rows: the ring part full (a third), just full (pos 0), wrapped (pos != 0)."""
    full = CAP // stride_of(nets)
    return dict(part=full // 3, full=full, wrapped=full + 5)[state]


def ring_fixture(nets, state, integer_rewards=False, seed=3):
    """A RingModel of CAP slots after pushes of ENVS envs x nets robots, as the trainer pushes them:
    row env * nets + robot, the env's team reward and done flag in every robot's row. Rewards random
    f32 (or integers, |r| <= 3), done with probability 0.2, s / s2 / a recognisable per row."""
    rng = np.random.RandomState(100 * nets + seed + 10 * STATES.index(state))
    ring = RingModel(CAP)
    n = stride_of(nets)
    for p in range(pushes_of(nets, state)):
        tag = 1000 * (p + 1) + np.arange(n)
        w = np.arange(OBS_WORDS)[None, :]
        r_env = rng.randint(-3, 4, ENVS).astype(np.float64) if integer_rewards else rng.randn(ENVS) * 30
        done_env = (rng.rand(ENVS) < 0.2).astype(np.uint8)
        ring.push((tag[:, None] * 16 + w).astype(np.int32), (tag[:, None] * 16 + w + 8 * 65536).astype(np.int32),
                  (tag % 5).astype(np.int32), r_env, done_env, n, nets,
                  s2_term=(tag[:, None] * 16 + w + 9 * 65536).astype(np.int32))
    return ring


def np_sample_nstep_agents(ring, B, nets, joint, seed, offset, base, count, stride, n_step, gamma):
    """evx_replay_sample_nstep_agents on a RingModel (or anything with its arrays and draws): rows
    [g B, (g + 1) B) are agent g's. Returns s, a, s2, r, done, gamma_row, len, idx as [nets * B] arrays."""
    smp = ring.sample_joint(B, nets, seed, offset) if joint else ring.sample_agents(B, nets, seed, offset)
    stride = min(stride, ring.capacity)
    R, G, D, S2, L = np_nstep(ring.r, ring.done, ring.s2, smp["idx"], base, count, stride, n_step, gamma)
    return dict(s=smp["s"], a=smp["a"], s2=S2, r=R, done=D, gamma_row=G, len=L, idx=smp["idx"])


def row_kinds(out, base, count, stride, n_step, cap=CAP):
    """How many rows of a restated batch end on (a done, the end of the range, full length), and how
    many have a successor that wrapped past the end of the ring."""
    L, D, idx = out["len"].astype(np.int64), out["done"], out["idx"]
    d0 = (idx - base) % cap
    by_done = int(((L < n_step) & (D != 0)).sum())
    cut = (L < n_step) & (D == 0)
    assert (d0[cut] + L[cut] * stride >= count).all()  # nothing else ends a chain early
    full = int(((L == n_step) & (n_step > 1)).sum())
    wrapped = int(((L > 1) & (idx + (L - 1) * stride >= cap)).sum())
    return by_done, int(cut.sum()), full, wrapped


# ------------------------------------------------------------------ the QMIX learn step with options
def host_ring(rp):
    """A RingModel holding a device ring's arrays, pos and size (evacx.trainer.Replay)."""
    ring = RingModel(rp.capacity)
    ring.s[:] = rp.s.cpu().numpy().reshape(-1, OBS_WORDS)
    ring.s2[:] = rp.s2.cpu().numpy().reshape(-1, OBS_WORDS)
    ring.a[:], ring.r[:], ring.done[:] = rp.a.cpu().numpy(), rp.r.cpu().numpy(), rp.done.cpu().numpy()
    ring.pos, ring.size = rp.pos, rp.size
    return ring


def qmix_opt_step_and_references(qm, lay, env, gb, r, d, huber_delta, gamma_row):
    """learn_util.qmix_step_and_references for one GroupedQMix step with double_q, the Huber loss and
    gamma_row, dropout off (drop_p = 0): the agents through float64_reference's gated network, both
    mixers and the loss in float64 under one autograd backward, clip_grad_norm_(1.0) and one Adam step
    per agent and for the mixer. The bootstrap actions of the reference are the device's (A.last_sel);
    ref.q2 is the online nets' float64 Q at s2 [n][B][5] from the parameters before the step, for the
    caller to judge those actions."""
    import torch

    import learn_util as lu
    A = qm.A
    n, B = A.G, gb.B
    assert A.drop_p == 0
    online = [A.online[j].state_dict() for j in range(n)]
    target = [A.target[j].state_dict() for j in range(n)]
    m, v, step = A.m.clone(), A.v.clone(), A.adam_step
    mix0, mixt0 = lu.mixer_dict(qm.mix, n), lu.mixer_dict(qm.mix_t, n)
    mix_adam = (qm.mix_m.clone(), qm.mix_v.clone(), qm.mix_step, qm.mix_lr)
    stream = A.drop_stream + 3  # double_q: one stream more than the forward pair's two
    loss = qm(lay.c, gb.s, gb.a, r, d, gb.s2, B, double_q=True, huber_delta=huber_delta, gamma_row=gamma_row)
    torch.cuda.synchronize()
    assert A.drop_stream == stream and A.last_sel is not None and A.last_sel.numel() == n * B
    sel = A.last_sel.clone().view(n, B).long()
    assert bool(((sel >= 0) & (sel < 5)).all())
    params = [{k: torch.nn.Parameter(t.double()) for k, t in sd.items()} for sd in online]
    mixp = {k: torch.nn.Parameter(t) for k, t in mix0.items()}
    ones = torch.ones(n * B, 512, dtype=torch.uint8, device=loss.device)
    qs, qts, q2 = [], [], []
    for j in range(n):
        bt = lu.net_batch(gb, j, ones, ones)
        g1, g2 = lu.net_gates(A._ws["h1"], A._ws["h2"], j, B)
        X, X2 = lu.expand64(env, bt.s_obs, B), lu.expand64(env, bt.s2_obs, B)
        qs.append(lu.torch_q_gated(params[j], X, g1, g2, 1.0)[0].gather(1, bt.a.long().unsqueeze(1)).squeeze(1))
        with torch.no_grad():
            qt = lu.torch_q({k: t.double() for k, t in target[j].items()}, X2, None, 1.0)
            qts.append(qt.gather(1, sel[j].unsqueeze(1)).squeeze(1))
            q2.append(lu.torch_q({k: t.double() for k, t in online[j].items()}, X2, None, 1.0))
    with torch.no_grad():
        y = r.double() + gamma_row.double() * lu.mixer64(mixt0, torch.stack(qts, 1)) * (~d.bool())
    ref = lu.SimpleNamespace(agents=[], q2=torch.stack(q2))
    dd = lu.mixer64(mixp, torch.stack(qs, 1)) - y
    ad = dd.abs()
    ref.within = int((ad <= huber_delta).sum())
    ref_loss = torch.where(ad <= huber_delta, 0.5 * dd * dd, huber_delta * (ad - 0.5 * huber_delta)).mean()
    ref_loss.backward()
    ref.loss = ref_loss.item()
    dev = lu.SimpleNamespace(loss=loss.item(), agents=[], mix_norm=qm.mix_norm.item(), mix=qm.mix.clone(), sel=sel)
    for j in range(n):
        rj = lu.SimpleNamespace()
        lu.clip_and_adam(params[j], (m[j], v[j], step, A.lr), rj)
        ref.agents.append(rj)
        dev.agents.append(lu.SimpleNamespace(norm=A.norm[j].item(), grads=A.grads[j].state_dict(),
                                             params=A.online[j].state_dict()))
    rm = lu.SimpleNamespace()
    lu.clip_and_adam(mixp, mix_adam, rm)
    ref.mix_norm, ref.mix = rm.norm, torch.cat([t.reshape(-1) for t in rm.params.values()])
    return dev, ref
