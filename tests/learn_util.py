"""Shared helpers of the learn-step tests (not a test module): the torch restatements of the MLP
Q-network and one fused x3 learn step next to its torch float64 reference.

Device side: Learner(kind="mlp", precision="f32") through learn_obs -- evx_qmlp_forward2,
evx_qmlp_td_backward_opt / _ss (qbwd3, bwd_mid, gemm_tn, reduce2), evx_qmlp_adam_pack3
(csrc/qmlp.hip) -- from compact observations with explicit dropout keep masks.
Reference side: DQNAgent.learn (agents/dqn_agent.py:126-168) in float64 on the expanded 726-column
observations with the same masks, parameters and Adam moments: loss, autograd, clip_grad_norm_(1.0),
one Adam(lr = 1e-3) step. It walks the device's own ReLU / dropout branch pattern (read from the
H1 planes and H2 the forward saved), so its arithmetic is comparable element by element; the loss and
the gradient norm are also taken with plain torch, and the branches that differ are returned.

Grouped nets (evacx.qgroup, evx_qmlp_*_g): one GroupedLearner step next to one such reference per net
on that net's rows, parameters, moments, keep masks (restated with oracle.dropout_keep) and gates; one
GroupedQMix step next to the agents, both mixers and the MSE in float64 under one autograd backward."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

GAMMA, KEEP = 0.99, 0.8


def torch_q(sd, X, mask, keep=KEEP):
    h = F.relu(F.linear(X, sd["fc1.weight"], sd["fc1.bias"]))
    if mask is not None:
        h = h * mask.to(X.dtype) / keep
    h = F.relu(F.linear(h, sd["fc2.weight"], sd["fc2.bias"]))
    return F.linear(h, sd["fc3.weight"], sd["fc3.bias"])


def torch_q_gated(sd, X, g1, g2, keep=KEEP):
    """The same network with the ReLU/dropout pattern given (g1: keep AND fc1 > 0, g2: fc2 > 0) --
    the device's own pattern, so autograd walks the branches the device's backward walked."""
    z1 = F.linear(X, sd["fc1.weight"], sd["fc1.bias"])
    h1 = z1 * g1 / keep
    z2 = F.linear(h1, sd["fc2.weight"], sd["fc2.bias"])
    return F.linear(z2 * g2, sd["fc3.weight"], sd["fc3.bias"]), z1, z2


@functools.lru_cache(maxsize=2)
def small_env(rows, R=4, grid=48, people=300, steps=7):
    """(layout, env) of a small env with at least `rows` robot rows a few random steps into its
    episodes (tests/test_qmlp_x3_gpu.py::_env_obs). The learn chain's dispatch depends on the batch
    size alone, not on the layout. Cached: the cases of a module share one env and never write it."""
    from evacx.env import DeviceLayout, VecEnv
    from evacx.layout import build_tables, synthetic
    E = (rows + R - 1) // R
    lay = DeviceLayout(build_tables(synthetic(grid, grid, R)), people)
    env = VecEnv(lay, E)
    env.seed([77 + i for i in range(E)])
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(steps):
        env.step(torch.randint(0, 5, (E * R,), device="cuda", dtype=torch.int32, generator=g))
    torch.cuda.synchronize()
    return lay, env


def attach_tables(lr, lay):
    """Both nets' act tables over Map.robot_range's columns, as VecTrainer attaches them."""
    c = lay.c
    for fast in (lr.fast, lr.fast_t):
        fast.attach_static(c, c.L, c.W, c.t_max, x_range=(max(c.rx_lo, 0), min(c.rx_hi, c.L + 1)))


def make_batch(env, lay, B, gen, table=False, weights=False, td_abs=False):
    """A learn batch: s and s' rows drawn without replacement from the env's observations, actions,
    rewards, done flags, both dropout keep masks; optionally importance weights and a |TD| buffer.
    table: three quarters of the s and of the s' rows moved to the layout's last fire step (the rows
    the act tables serve). gen: a CPU generator (the draws do not depend on the device)."""
    from evacx.qmlp import HID
    dev = env.obs.device
    obs = env.obs.view(-1, 8)
    assert obs.shape[0] >= 2 * B
    perm = torch.randperm(obs.shape[0], generator=gen)
    s_obs = obs[perm[:B].to(dev)].contiguous()
    s2_obs = obs[perm[B:2 * B].to(dev)].contiguous()
    if table:
        s_obs[:3 * B // 4, 6] = int(lay.c.t_max)
        s2_obs[B // 4:, 6] = int(lay.c.t_max)
    bt = SimpleNamespace(B=B, s_obs=s_obs.view(-1), s2_obs=s2_obs.view(-1))
    bt.a = torch.randint(0, 5, (B,), generator=gen, dtype=torch.int32).to(dev)
    bt.r = (torch.randn(B, generator=gen) * 30).to(dev)
    bt.d = (torch.rand(B, generator=gen) < 0.05).to(torch.uint8).to(dev)
    bt.m1 = (torch.rand(B, HID, generator=gen) >= 0.2).to(torch.uint8).to(dev)
    bt.m2 = (torch.rand(B, HID, generator=gen) >= 0.2).to(torch.uint8).to(dev)
    bt.w = (0.1 + 0.9 * torch.rand(B, generator=gen)).to(dev) if weights else None
    bt.td_abs = torch.full((B,), float("nan"), device=dev) if td_abs else None
    return bt


def expand64(env, obs, B):
    """[B][726] float64 of B compact observations (expand_obs takes whole envs: padded, then cut)."""
    from evacx.qmlp import K1
    R = env.lay.R
    pad = (-B) % R
    ob = obs.view(B, 8)
    if pad:
        ob = torch.cat([ob, ob[:1].expand(pad, 8)]).contiguous()
    return env.expand_obs(torch.float64, ob.view(-1)).reshape(B + pad, K1)[:B]


def device_gates(h1, h2, B):
    """The device's branch pattern from the forward it saved: g1 = H1 > 0 (hi + lo planes: keep AND
    fc1 > 0), g2 = H2 > 0, as float64."""
    from evacx.qmlp import HID, HID2
    p = h1[:2 * B * HID].view(torch.bfloat16).view(2, B, HID).float()
    return ((p[0] + p[1]) > 0).double(), (h2.reshape(-1)[:B * HID2].view(B, HID2) > 0).double()


def float64_reference(env, online_sd, target_sd, bt, g1, g2, adam=None, keep=KEEP):
    """DQNAgent.learn in float64 on bt from the given f32 parameters. adam = (m, v, step, lr): the
    flat f32 moments and the step count BEFORE this step; with it the gradients are clipped to norm 1
    and one Adam step is taken (ref.params), without it the raw gradients are returned.
    Returns a namespace: loss, norm, grads (through the device's gates g1, g2); plain_loss, plain_norm
    (torch's own branches); td_abs; flips = per layer (differing branches, max |z| among them,
    max |z| of the layer, activations). keep: 1 - the dropout probability (1.0 with masks of ones:
    dropout off)."""
    B = bt.B
    X, X2 = expand64(env, bt.s_obs, B), expand64(env, bt.s2_obs, B)
    params = {k: torch.nn.Parameter(v.detach().double().clone()) for k, v in online_sd.items()}
    tgt = {k: v.detach().double() for k, v in target_sd.items()}
    ai = bt.a.long().unsqueeze(1)
    w = None if bt.w is None else bt.w.double()

    def loss_of(q, y):
        e = (q.gather(1, ai).squeeze(1) - y) ** 2
        return (e if w is None else w * e).mean()
    ref = SimpleNamespace()
    with torch.no_grad():
        y = bt.r.double() + GAMMA * torch_q(tgt, X2, bt.m2, keep).max(1)[0] * (~bt.d.bool())
    # plain torch: loss, norm, and the branches it takes
    plain = {k: p.detach().clone().requires_grad_(True) for k, p in params.items()}
    ref.plain_loss = loss_of(torch_q(plain, X, bt.m1, keep), y)
    ref.plain_loss.backward()
    ref.plain_norm = torch.sqrt(sum((p.grad ** 2).sum() for p in plain.values())).item()
    ref.plain_loss = ref.plain_loss.item()
    qg, z1, _ = torch_q_gated(params, X, g1, g2, keep)
    with torch.no_grad():
        z2p = F.linear(F.relu(z1) * bt.m1.double() / keep, params["fc2.weight"], params["fc2.bias"])
        ref.flips = []
        for z, f in ((z1, ((z1 > 0) & bt.m1.bool()) != g1.bool()), (z2p, (z2p > 0) != g2.bool())):
            n = int(f.sum())
            ref.flips.append((n, z[f].abs().max().item() if n else 0.0, z.abs().max().item(), f.numel()))
        ref.td_abs = (qg.gather(1, ai).squeeze(1) - y).abs()
    loss = loss_of(qg, y)
    loss.backward()
    ref.loss = loss.item()
    if adam is None:
        ref.norm = torch.sqrt(sum((p.grad ** 2).sum() for p in params.values())).item()
        ref.grads = {k: p.grad.clone() for k, p in params.items()}
        return ref
    clip_and_adam(params, adam, ref)
    return ref


def clip_and_adam(params, adam, ref):
    """clip_grad_norm_(1.0) and one Adam step on the float64 `params` (a dict in state_dict order whose
    .grad are set) from adam = (m, v, step, lr), the flat f32 moments and the step count before this
    step. Fills ref.norm (before clipping), ref.grads (clipped) and ref.params."""
    m, v, step, lr = adam
    opt = torch.optim.Adam(params.values(), lr=lr, foreach=False)
    o = 0
    for p in params.values():  # the same moments: state_dict order, as the flat buffers
        n = p.numel()
        opt.state[p] = dict(step=torch.tensor(float(step)), exp_avg=m[o:o + n].double().view_as(p).clone(),
                            exp_avg_sq=v[o:o + n].double().view_as(p).clone())
        o += n
    ref.norm = torch.nn.utils.clip_grad_norm_(params.values(), 1.0).item()
    ref.grads = {k: p.grad.clone() for k, p in params.items()}
    opt.step()
    ref.params = {k: p.detach() for k, p in params.items()}


def learn_step_and_reference(lr, lay, env, bt):
    """One fused x3 learn step of `lr` on bt and its float64 reference from the same parameters and
    Adam moments. Returns (dev, ref): dev.loss, dev.norm, dev.grads (clipped), dev.params, dev.td_abs."""
    from evacx.qmlp import HID, HID2
    assert lr.fast is not None and lr.fast.x3 and lr.fused_opt  # the trainer's chain
    B = bt.B
    online_sd, target_sd = lr.online.state_dict(), lr.target.state_dict()
    adam = (lr.m.clone(), lr.v.clone(), lr.adam_step, lr.lr)
    loss = lr.learn_obs(lay.c, bt.s_obs, bt.a, bt.r, bt.d, bt.s2_obs, B, weights=bt.w, td_abs=bt.td_abs,
                        mask_online=bt.m1, mask_target=bt.m2)
    torch.cuda.synchronize()
    dev_ = torch.device("cuda")
    g1, g2 = device_gates(lr.net.ws.get("fh1", (B * 2 * HID,), torch.int16, dev_),
                          lr.net.ws.get("fh2", (B * HID2,), torch.float32, dev_), B)
    dev = SimpleNamespace(loss=loss.item(), norm=lr.norm.item(), grads=lr.grads.state_dict(),
                          params=lr.online.state_dict(), td_abs=bt.td_abs)
    return dev, float64_reference(env, online_sd, target_sd, bt, g1, g2, adam)


def check_flips(ref, what=""):
    """The branches that differ from plain torch's are roundings of 0: each within 1e-4 of its
    layer's max |z|, at most max(2, 1e-5 x activations) of them (per layer and in all)."""
    for n, zmax_f, zmax, _ in ref.flips:
        if n:
            print(f"{what}: {n} branches differ, |z| <= {zmax_f:.3e} of max {zmax:.3e}")
    for n, zmax_f, zmax, numel in ref.flips:
        assert zmax_f <= 1e-4 * zmax, (what, n, zmax_f, zmax)
        assert n <= max(2, 1e-5 * numel), (what, n, numel)
    assert sum(f[0] for f in ref.flips) <= max(2, 1e-5 * sum(f[3] for f in ref.flips)), (what, ref.flips)


def check_loss_and_grads(dev, ref, what=""):
    """The x3 bars on loss, norm, gradients and |TD| (tests/test_qmlp_x3_gpu.py,
    test_bench_scale_gpu.py::test_x3_learn_at_bench_batch). Prints every figure before asserting."""
    fig = [f"loss {dev.loss:.9g} ref {ref.loss:.9g} plain {ref.plain_loss:.9g}",
           f"norm {dev.norm:.9g} ref {ref.norm:.9g} plain {ref.plain_norm:.9g}"]
    for k, r in ref.grads.items():
        e = (dev.grads[k].double() - r).abs()
        fig.append(f"grad {k}: max err {e.max().item():.3e}, max |ref| {r.abs().max().item():.3e}, worst "
                   f"err / (2e-3 |ref| + atol) {(e / (2e-3 * r.abs() + 1e-5 * r.abs().max() + 1e-9)).max().item():.3f}")
    print(what + ": " + "; ".join(fig))
    assert all(torch.isfinite(g).all() for g in dev.grads.values()) and dev.loss == dev.loss, what
    assert abs(dev.loss - ref.loss) <= 2e-4 * abs(ref.loss) + 1e-5, (what, dev.loss, ref.loss)
    assert abs(dev.loss - ref.plain_loss) <= 2e-4 * abs(ref.plain_loss) + 1e-5, (what, dev.loss, ref.plain_loss)
    assert abs(dev.norm - ref.norm) <= 2e-4 * ref.norm, (what, dev.norm, ref.norm)
    assert abs(dev.norm - ref.plain_norm) <= 1e-3 * ref.plain_norm, (what, dev.norm, ref.plain_norm)
    for k, r in ref.grads.items():
        torch.testing.assert_close(dev.grads[k].double(), r, rtol=2e-3, atol=1e-5 * r.abs().max().item() + 1e-9,
                                   msg=lambda m, k=k: f"{what} grad {k}: {m}")
    if dev.td_abs is not None:
        torch.testing.assert_close(dev.td_abs.double(), ref.td_abs, rtol=2e-4, atol=2e-5,
                                   msg=lambda m: f"{what} td_abs: {m}")


def check_adam(dev, ref, what=""):
    """At most 1e-3 of a tensor's elements off by more than 1e-5, none by more than 2e-3."""
    for k, r in ref.params.items():
        diff = (dev.params[k].double() - r).abs()
        frac, worst = (diff > 1e-5).double().mean().item(), diff.max().item()
        print(f"{what} adam {k}: {frac:.2e} of the elements beyond 1e-5, max {worst:.3e}")
        assert frac <= 1e-3, (what, k, frac, worst)
        assert worst <= 2e-3, (what, k, worst)


# ------------------------------------------------------------------ grouped nets (evacx.qgroup)
def grouped_batch(env, G, B, gen, p_done=0.1):
    """G x B transitions for G nets, net g's on rows [g B, (g + 1) B): s and s' drawn with
    replacement from the env's observations (tests/test_qgroup_gpu.py::_batch: the env's row count
    does not limit G x B), actions, rewards, done flags. gen: a CPU generator."""
    dev = env.obs.device
    obs = env.obs.view(-1, 8)
    n = obs.shape[0]
    gb = SimpleNamespace(G=G, B=B)
    gb.s = obs[torch.randint(0, n, (G * B,), generator=gen).to(dev)].contiguous().view(-1)
    gb.s2 = obs[torch.randint(0, n, (G * B,), generator=gen).to(dev)].contiguous().view(-1)
    gb.a = torch.randint(0, 5, (G * B,), generator=gen, dtype=torch.int32).to(dev)
    gb.r = (torch.randn(G * B, generator=gen) * 30).to(dev)
    gb.d = (torch.rand(G * B, generator=gen) < p_done).to(torch.uint8).to(dev)
    return gb


def grouped_keep_masks(seed, stream, p, G, B, dev):
    """The grouped forward pair's dropout keep masks [G B][512] uint8, restated on the host
    (oracle.dropout_keep): the online net's on `stream`, the target net's on `stream + 1`, the hash
    rows of net g being [g B, (g + 1) B) (fwd_net: drop_row0 + g B). p = 0: all ones."""
    from evacx.qmlp import HID
    if p <= 0:
        ones = torch.ones(G * B, HID, dtype=torch.uint8, device=dev)
        return ones, ones
    from oracle import oracle
    return tuple(torch.from_numpy(oracle.dropout_keep(seed, stream + k, p, G * B, HID)).to(dev) for k in (0, 1))


def net_batch(gb, g, m1, m2):
    """Net g's rows of a grouped batch as float64_reference's batch (no weights, no |TD| out)."""
    B = gb.B
    rows = slice(g * B, (g + 1) * B)
    return SimpleNamespace(B=B, s_obs=gb.s.view(-1, 8)[rows].contiguous().view(-1),
                           s2_obs=gb.s2.view(-1, 8)[rows].contiguous().view(-1), a=gb.a[rows], r=gb.r[rows], d=gb.d[rows],
                           m1=m1[rows], m2=m2[rows], w=None, td_abs=None)


def net_gates(h1, h2, g, B):
    """device_gates of net g's slice of the grouped forward's saved [G][2][B][512] H1 planes and
    [G][B][256] H2."""
    from evacx.qmlp import HID, HID2
    return device_gates(h1[g * 2 * B * HID:(g + 1) * 2 * B * HID], h2.reshape(-1)[g * B * HID2:(g + 1) * B * HID2], B)


def grouped_step_and_references(grp, lay, env, gb):
    """One GroupedLearner.learn_obs step on gb and, per net, float64_reference on that net's rows from
    that net's parameters, target parameters and Adam moments before the step, its slice of the
    dropout keep masks and the device's own gates from its slice of the saved H1 planes and H2.
    Returns [(dev, ref)] per net, as learn_step_and_reference's pair."""
    G, B = grp.G, gb.B
    assert G == gb.G
    online = [grp.online[g].state_dict() for g in range(G)]
    target = [grp.target[g].state_dict() for g in range(G)]
    m, v, step = grp.m.clone(), grp.v.clone(), grp.adam_step
    stream = grp.drop_stream + 2  # learn_obs advances the stream, then draws on it and the next
    loss = grp.learn_obs(lay.c, gb.s, gb.a, gb.r, gb.d, gb.s2, B)
    torch.cuda.synchronize()
    assert grp.drop_stream == stream and grp.adam_step == step + 1
    loss, norm = loss.clone(), grp.norm.clone()
    m1, m2 = grouped_keep_masks(grp.seed, stream, grp.drop_p, G, B, loss.device)
    out = []
    for g in range(G):
        g1, g2 = net_gates(grp._ws["h1"], grp._ws["h2"], g, B)
        ref = float64_reference(env, online[g], target[g], net_batch(gb, g, m1, m2), g1, g2,
                                (m[g], v[g], step, grp.lr), keep=1.0 - grp.drop_p)
        dev = SimpleNamespace(loss=loss[g].item(), norm=norm[g].item(), grads=grp.grads[g].state_dict(),
                              params=grp.online[g].state_dict(), td_abs=None)
        out.append((dev, ref))
    return out


def mixer64(sd, q):
    """MixingNetwork.forward (runners/train_qmix.py:39-54) on a dict of its parameters."""
    hidden = torch.relu(q @ sd["fc1_weight"].abs() + sd["fc1_bias"])
    return (hidden @ sd["fc2_weight"].abs() + sd["fc2_bias"]).squeeze(-1)


def mixer_dict(flat, n, embed=32):
    """A flat mixer buffer (state_dict order) as a dict of float64 tensors."""
    f = flat.detach().double()
    o = [0, n * embed, n * embed + embed, n * embed + 2 * embed, n * embed + 2 * embed + 1]
    return {"fc1_weight": f[o[0]:o[1]].view(n, embed).clone(), "fc1_bias": f[o[1]:o[2]].clone(),
            "fc2_weight": f[o[2]:o[3]].view(embed, 1).clone(), "fc2_bias": f[o[3]:o[4]].clone()}


def qmix_step_and_references(qm, lay, env, gb, r, d):
    """One GroupedQMix step (gb: the agents' rows as grouped_batch's, r / d [B]: the joint reward and
    done flag) and its float64 reference from the same state: the agents through float64_reference's
    gated network (the device's own gates, the restated keep masks), both mixers, the MSE, one autograd
    backward -- so each agent's output gradient is the float64 mixer's dQ -- then clip_grad_norm_(1.0)
    and one Adam step per agent and for the mixer. Returns (dev, ref): loss, agents [(dev, ref)] with
    norm / grads / params, mix_norm, mix (flat parameters after the step)."""
    A = qm.A
    n, B = A.G, gb.B
    online = [A.online[j].state_dict() for j in range(n)]
    target = [A.target[j].state_dict() for j in range(n)]
    m, v, step = A.m.clone(), A.v.clone(), A.adam_step
    mix0, mixt0 = mixer_dict(qm.mix, n), mixer_dict(qm.mix_t, n)
    mix_adam = (qm.mix_m.clone(), qm.mix_v.clone(), qm.mix_step, qm.mix_lr)
    stream = A.drop_stream + 2
    loss = qm(lay.c, gb.s, gb.a, r, d, gb.s2, B)
    torch.cuda.synchronize()
    assert A.drop_stream == stream
    keep = 1.0 - A.drop_p
    m1, m2 = grouped_keep_masks(A.seed, stream, A.drop_p, n, B, loss.device)
    params = [{k: torch.nn.Parameter(t.double()) for k, t in sd.items()} for sd in online]
    mixp = {k: torch.nn.Parameter(t) for k, t in mix0.items()}
    qs, qts = [], []
    for j in range(n):
        bt = net_batch(gb, j, m1, m2)
        g1, g2 = net_gates(A._ws["h1"], A._ws["h2"], j, B)
        X, X2 = expand64(env, bt.s_obs, B), expand64(env, bt.s2_obs, B)
        qs.append(torch_q_gated(params[j], X, g1, g2, keep)[0].gather(1, bt.a.long().unsqueeze(1)).squeeze(1))
        with torch.no_grad():
            qts.append(torch_q({k: t.double() for k, t in target[j].items()}, X2, bt.m2, keep).max(1)[0])
    with torch.no_grad():
        y = r.double() + A.gamma * mixer64(mixt0, torch.stack(qts, 1)) * (~d.bool())
    ref = SimpleNamespace(agents=[])
    ref_loss = ((mixer64(mixp, torch.stack(qs, 1)) - y) ** 2).mean()
    ref_loss.backward()
    ref.loss = ref_loss.item()
    dev = SimpleNamespace(loss=loss.item(), agents=[], mix_norm=qm.mix_norm.item(), mix=qm.mix.clone())
    for j in range(n):
        rj = SimpleNamespace()
        clip_and_adam(params[j], (m[j], v[j], step, A.lr), rj)
        ref.agents.append(rj)
        dev.agents.append(SimpleNamespace(norm=A.norm[j].item(), grads=A.grads[j].state_dict(),
                                          params=A.online[j].state_dict()))
    rm = SimpleNamespace()
    clip_and_adam(mixp, mix_adam, rm)
    ref.mix_norm, ref.mix = rm.norm, torch.cat([t.reshape(-1) for t in rm.params.values()])
    return dev, ref
