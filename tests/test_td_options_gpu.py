"""Double-Q targets, the Huber loss and soft target updates on the GPU (evx_td_loss_opt,
evx_qmlp_td_backward_opt, evx_polyak, evx_qmlp_polyak_pack3, Learner / VecTrainer / DQNAgent).

The reference has none of the three (agents/dqn_agent.py:143-151 is the max target with the MSE
and a hard copy), so they are pinned by restatements here: numpy float32 in the kernels' stated
order of operations, and torch autograd in fp32. Bars: a per-row f32 result within 1 ulp of the
restatement, a mean loss rtol 2e-4 (the project's loss bar), learn steps as
tests/test_qmlp_x3_gpu.py / tests/test_qnet_gpu.py state them."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _env_obs(E, R=4, steps=7, grid=48, people=300):
    from evacx.env import DeviceLayout, VecEnv
    from evacx.layout import build_tables, synthetic
    lay = DeviceLayout(build_tables(synthetic(grid, grid, R)), people)
    env = VecEnv(lay, E)
    env.seed([77 + i for i in range(E)])
    env.reset()
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(steps):
        env.step(torch.randint(0, 5, (E * R,), device=DEV, dtype=torch.int32, generator=g))
    torch.cuda.synchronize()
    return lay, env


@pytest.fixture(scope="module")
def small_env():
    _need_gpu()
    return _env_obs(E=160)


def torch_q(sd, X, mask):
    """agents/dqn_agent.py:40-61's fc stack on the flattened observation (the MLP variant)."""
    h = F.relu(F.linear(X, sd["fc1.weight"], sd["fc1.bias"]))
    if mask is not None:
        h = h * mask.float() / 0.8
    h = F.relu(F.linear(h, sd["fc2.weight"], sd["fc2.bias"]))
    return F.linear(h, sd["fc3.weight"], sd["fc3.bias"])


def _batch(env, lay, B, g, n_masks=3):
    """B rows of s and s' from the env's observations, actions, rewards randn * 30, 20 % done
    flags and explicit keep masks, all from the seeded CPU generator g."""
    from evacx.qmlp import HID
    perm = torch.randperm(env.E * lay.R, generator=g)
    obs = env.obs.view(-1, 8)
    s_obs = obs[perm[:B].to(DEV)].contiguous().view(-1)
    s2_obs = obs[perm[B:2 * B].to(DEV)].contiguous().view(-1)
    a = torch.randint(0, 5, (B,), generator=g, dtype=torch.int32).to(DEV)
    r = (torch.randn(B, generator=g) * 30).to(DEV)
    d = (torch.rand(B, generator=g) < 0.2).to(torch.uint8).to(DEV)
    masks = [(torch.rand(B, HID, generator=g) >= 0.2).to(torch.uint8).to(DEV) for _ in range(n_masks)]
    return s_obs, s2_obs, a, r, d, masks


# ------------------------------------------------------------------ 5. the TD kernel
def np_td(Q, Qt, act, rew, done, gamma, B, sel, delta, w):
    """The per-row order of include/evacx.h's evx_td_opts comment in numpy float32 (every
    operation rounded to f32, no fused multiply-add); rows of one net. -> dq_at_action, |d|, l."""
    f = np.float32
    rows = np.arange(B)
    if sel is None:
        v = Qt.max(axis=1)
    else:
        v = Qt[rows, np.clip(sel, 0, Qt.shape[1] - 1)]
    flag = np.where(done != 0, f(0), f(1)).astype(f)
    y = rew + (f(gamma) * v) * flag
    d = Q[rows, act] - y
    ad = np.abs(d)
    if delta > 0:
        dl = f(delta)
        l = np.where(ad <= dl, f(0.5) * (d * d), dl * (ad - f(0.5) * dl)).astype(f)
        g = np.minimum(np.maximum(d, -dl), dl)
    else:
        l = d * d
        g = f(2) * d
    if w is not None:
        l = w * l
        g = w * g
    for x in (y, d, l, g):
        assert x.dtype == np.float32
    return g / f(B), ad, l


def _run_td(entry, Q, Qt, act, rew, done, B, nets, w, sel, delta, nzero=5000):
    """entry: "g" (evx_td_loss_zero_g), "null" (evx_td_loss_opt, opt = NULL) or "opt"."""
    from evacx.qmlp import td_opts
    from evacx._lib import check, lib
    L = lib()
    A = Q.shape[1]
    dQ = torch.full((nets * B, A), float("nan"), device=DEV)
    loss = torch.full((nets,), float("nan"), device=DEV)
    td_abs = torch.full((nets * B,), float("nan"), device=DEV)
    zero = torch.ones(nzero, device=DEV)
    ws = torch.zeros(int(L.evx_td_loss_ws_floats(B, nets)), device=DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    head = (p(Q), p(Qt), A, p(act), p(rew), p(done), 0.99, B, nets, p(w), p(dQ), p(loss), p(td_abs), p(zero), nzero,
            p(ws), ws.numel())
    if entry == "g":
        assert sel is None and delta == 0
        check(L.evx_td_loss_zero_g(*head, None), "td_loss_zero_g")
    else:
        o = td_opts(sel, delta)
        check(L.evx_td_loss_opt(*head, None if entry == "null" else C.byref(o), None), "td_loss_opt")
    torch.cuda.synchronize()
    return dQ, loss, td_abs, zero


def _ulp_close(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)


@pytest.mark.parametrize("B,nets", [(250, 1), (64, 3)])
def test_td_loss_opt_matches_numpy_float32(B, nets):
    """evx_td_loss_opt for every combination of sel, Huber delta and weights against the numpy
    float32 restatement: dQ exactly zero off the taken action, dQ at the action and |d| within
    1 ulp, the loss rtol 2e-4 of the float64 mean of the per-row terms. B = 250: a partial
    block; nets = 3: the grouped rows."""
    _need_gpu()
    g = torch.Generator().manual_seed(100 + B)
    n, A = nets * B, 5
    Q = (torch.randn(n, A, generator=g) * 3).to(DEV)
    Qt = (torch.randn(n, A, generator=g) * 3).to(DEV)
    act = torch.randint(0, A, (n,), generator=g, dtype=torch.int32).to(DEV)
    rew = (torch.randn(n, generator=g) * 30).to(DEV)
    done = (torch.rand(n, generator=g) < 0.2).to(torch.uint8).to(DEV)
    sel_r = torch.randint(0, A, (n,), generator=g, dtype=torch.int32).to(DEV)
    w_r = (torch.rand(n, generator=g) * 0.9 + 0.1).to(DEV)
    Qn, Qtn, an, rn, dn = (t.cpu().numpy() for t in (Q, Qt, act, rew, done))
    for sel in (None, sel_r):
        for delta in (0.0, 10.0):
            for w in (None, w_r):
                dQ, loss, td_abs, zero = _run_td("opt", Q, Qt, act, rew, done, B, nets, w, sel, delta)
                assert torch.count_nonzero(zero) == 0
                dQn, tdn, lossn = dQ.cpu().numpy(), td_abs.cpu().numpy(), loss.cpu().numpy()
                for k in range(nets):
                    r0 = slice(k * B, (k + 1) * B)
                    gref, adref, lref = np_td(Qn[r0], Qtn[r0], an[r0], rn[r0], dn[r0], 0.99, B,
                                              None if sel is None else sel.cpu().numpy()[r0], delta,
                                              None if w is None else w.cpu().numpy()[r0])
                    if delta > 0:  # both Huber branches, judged on the reference alone
                        inner = float((adref <= 10).mean())
                        assert 0.1 <= inner <= 0.9, inner
                    rows = np.arange(B)
                    got = dQn[r0]
                    off = np.ones_like(got, dtype=bool)
                    off[rows, an[r0]] = False
                    assert (got[off] == 0).all()
                    tag = (sel is not None, delta, w is not None, k)
                    assert _ulp_close(got[rows, an[r0]], gref).all(), tag
                    assert _ulp_close(tdn[r0], adref).all(), tag
                    want = float(lref.astype(np.float64).mean())
                    assert abs(float(lossn[k]) - want) <= 2e-4 * abs(want), (tag, float(lossn[k]), want)


@pytest.mark.parametrize("B,nets", [(250, 1), (64, 3)])
def test_td_loss_opt_off_is_the_existing_entry_and_sel_is_clamped(B, nets):
    _need_gpu()
    g = torch.Generator().manual_seed(7 + B)
    n, A = nets * B, 5
    Q = (torch.randn(n, A, generator=g) * 3).to(DEV)
    Qt = (torch.randn(n, A, generator=g) * 3).to(DEV)
    act = torch.randint(0, A, (n,), generator=g, dtype=torch.int32).to(DEV)
    rew = (torch.randn(n, generator=g) * 30).to(DEV)
    done = (torch.rand(n, generator=g) < 0.2).to(torch.uint8).to(DEV)
    w = (torch.rand(n, generator=g) * 0.9 + 0.1).to(DEV)
    for ww in (None, w):
        base = _run_td("g", Q, Qt, act, rew, done, B, nets, ww, None, 0.0)
        for entry in ("null", "opt"):
            got = _run_td(entry, Q, Qt, act, rew, done, B, nets, ww, None, 0.0)
            for x, y in zip(got, base):
                assert torch.equal(x, y), entry
    # an index outside the row is clamped into it: nothing is read out of bounds
    def full(v):
        return torch.full((n,), v, dtype=torch.int32, device=DEV)
    for bad, good in ((-3, 0), (9, 4)):
        for delta in (0.0, 10.0):
            a = _run_td("opt", Q, Qt, act, rew, done, B, nets, w, full(bad), delta)
            b = _run_td("opt", Q, Qt, act, rew, done, B, nets, w, full(good), delta)
            for x, y in zip(a, b):
                assert torch.isfinite(x).all() and torch.equal(x, y), (bad, delta)


# ------------------------------------------------------------------ 6. fused == separate
@pytest.mark.parametrize("hook", [False, True])
def test_fused_learn_chain_matches_separate_launches_with_options(small_env, hook):
    """tests/test_qmlp_x3_gpu.py::test_fused_learn_chain_matches_separate_launches with
    double_q, the Huber loss (delta 10) on, B = 256: evx_qmlp_td_backward_opt against
    evx_td_loss_opt + the separate backward, that test's bars; the selected actions equal."""
    from evacx.qnet import Learner
    lay, env = small_env
    B = 256
    runs = []
    for fused in (False, True, True):
        lr = Learner(kind="mlp", precision="f32", seed=33, lr=1e-3, double_q=True, loss="huber", huber_delta=10)
        assert lr.fused_opt
        lr.fused_opt = fused
        if hook:
            lr.grad_hook = lambda g: g.mul_(1.0)
        g = torch.Generator().manual_seed(9)
        for it in range(3):
            s_obs, s2_obs, a, r, d, (m1, m2, m3) = _batch(env, lay, B, g)
            loss = lr.learn_obs(lay.c, s_obs, a, r, d, s2_obs, B, mask_online=m1, mask_target=m2, mask_select=m3)
        torch.cuda.synchronize()
        runs.append(dict(loss=loss.item(), norm=lr.norm.item(), sel=lr.last_sel.clone(),
                         grads={k: v.clone() for k, v in lr.grads.state_dict().items()},
                         params={k: v.clone() for k, v in lr.online.state_dict().items()}))
    sep, fus, fus2 = runs
    assert fus["loss"] == fus2["loss"] and fus["norm"] == fus2["norm"]
    assert torch.equal(fus["sel"], fus2["sel"])
    for k in fus["params"]:
        assert torch.equal(fus["grads"][k], fus2["grads"][k]), k
        assert torch.equal(fus["params"][k], fus2["params"][k]), k
    assert sep["sel"].dtype == torch.int32 and sep["sel"].numel() == B
    assert torch.equal(sep["sel"], fus["sel"])
    assert abs(sep["loss"] - fus["loss"]) <= 1e-5 * abs(sep["loss"]) + 1e-7
    assert abs(sep["norm"] - fus["norm"]) <= 1e-5 * sep["norm"] + 1e-9
    for k in sep["params"]:
        scale = sep["grads"][k].abs().max().item()
        torch.testing.assert_close(fus["grads"][k], sep["grads"][k], rtol=1e-4, atol=1e-6 * scale + 1e-12)
        torch.testing.assert_close(fus["params"][k], sep["params"][k], rtol=1e-5, atol=2e-6)


# ------------------------------------------------------------------ 7. against torch autograd
def _check_selection(sel_dev, q_ref, agree_bar):
    """The device's greedy actions against the reference's Q: agreement >= agree_bar, every row
    that differs a near-tie of the reference (top-two gap <= twice the Q bar), and the reference
    alone has at most 0.5 % of such near-ties (else: change the seed, not the bar)."""
    sel_ref = q_ref.argmax(1)
    top2 = q_ref.topk(2, dim=1)[0]
    gap = top2[:, 0] - top2[:, 1]
    bar = 2 * (2e-4 * q_ref.abs().max(1)[0] + 2e-5)
    assert (gap <= bar).float().mean().item() <= 0.005, "the reference has near-ties: change the seed"
    differ = sel_dev.long() != sel_ref
    assert (~differ).float().mean().item() >= agree_bar
    assert (gap[differ] <= bar[differ]).all()


@pytest.mark.parametrize("loss_kind", ["huber", "mse"])
def test_x3_learn_steps_with_options_match_torch_autograd(small_env, loss_kind):
    """tests/test_qmlp_x3_gpu.py::test_x3_learn_steps_match_torch_adam with double_q (and the
    Huber loss): the target is the target net's value of the online net's greedy action at s'.
    The loss and gradient reference takes the device's own selection, so a near-tie of the
    selection does not leak into those bars; the selection has its own check."""
    from evacx.qmlp import K1
    from evacx.qnet import Learner
    lay, env = small_env
    B = 256
    lr = Learner(kind="mlp", precision="f32", seed=21, lr=1e-3, double_q=True, loss=loss_kind, huber_delta=10)
    sd0 = {k: v.clone() for k, v in lr.online.state_dict().items()}
    params = {k: torch.nn.Parameter(v.clone()) for k, v in sd0.items()}
    tgt = {k: v.clone() for k, v in sd0.items()}
    opt = torch.optim.Adam(params.values(), lr=1e-3)
    g = torch.Generator().manual_seed(3)
    for it in range(3):
        if it > 0:  # each step compared from the same state (params + moments)
            lr.online.load_state_dict({k: p.detach() for k, p in params.items()})
            lr.fast.repack()
            for key, buf in (("exp_avg", lr.m), ("exp_avg_sq", lr.v)):
                buf.copy_(torch.cat([opt.state[p][key].reshape(-1) for p in params.values()]))
        s_obs, s2_obs, a, r, d, (m1, m2, m3) = _batch(env, lay, B, g)
        stream0 = lr.drop_stream
        loss = lr.learn_obs(lay.c, s_obs, a, r, d, s2_obs, B, mask_online=m1, mask_target=m2, mask_select=m3)
        assert lr.drop_stream == stream0 + 3
        sel = lr.last_sel.clone()
        X = env.expand_obs(torch.float32, s_obs).reshape(B, K1)
        X2 = env.expand_obs(torch.float32, s2_obs).reshape(B, K1)
        with torch.no_grad():
            _check_selection(sel, torch_q(params, X2, m3), 0.995)
            y = r + 0.99 * torch_q(tgt, X2, m2).gather(1, sel.long().unsqueeze(1)).squeeze(1) * (~d.bool())
        q = torch_q(params, X, m1).gather(1, a.long().unsqueeze(1)).squeeze(1)
        ref_loss = F.huber_loss(q, y, delta=10.0) if loss_kind == "huber" else F.mse_loss(q, y)
        opt.zero_grad()
        ref_loss.backward()
        gnorm = torch.nn.utils.clip_grad_norm_(params.values(), 1.0)
        grads_ref = {k: p.grad.clone() for k, p in params.items()}
        opt.step()
        torch.cuda.synchronize()
        assert abs(loss.item() - ref_loss.item()) <= 2e-4 * abs(ref_loss.item()) + 1e-5
        assert abs(lr.norm.item() - gnorm.item()) <= 2e-4 * gnorm.item() + 1e-6
        for k in params:
            ref = grads_ref[k]
            torch.testing.assert_close(lr.grads[k], ref, rtol=2e-3, atol=1e-5 * ref.abs().max().item() + 1e-9)
            diff = (lr.online[k] - params[k].detach()).abs()
            assert (diff > 1e-5).float().mean().item() <= 1e-3, (k, diff.max().item())
            assert diff.max().item() <= 2e-3, (k, diff.max().item())


# ------------------------------------------------------------------ 8. dense path
def _conv_forward(sd, x, mask):
    """agents/dqn_agent.py:35-61 with an injected dropout keep mask."""
    B = x.shape[0]
    h = x.permute(0, 3, 1, 2).contiguous()
    for c in ("conv1", "conv2", "conv3"):
        h = F.relu(F.conv2d(h, sd[c + ".weight"], sd[c + ".bias"], padding=1))
    h = F.relu(F.linear(h.reshape(B, -1), sd["fc1.weight"], sd["fc1.bias"]))
    h = h * mask.float() / 0.8
    h = F.relu(F.linear(h, sd["fc2.weight"], sd["fc2.bias"]))
    return F.linear(h, sd["fc3.weight"], sd["fc3.bias"])


def test_dense_learn_with_options_matches_torch_autograd():
    """Learner.learn (conv net, exact f32 GEMMs), B = 32, double_q + Huber against torch autograd
    on the CPU: the bars of tests/test_qnet_gpu.py::test_learn_steps_match_torch_adam (f32)."""
    _need_gpu()
    from evacx.qnet import Learner
    B = 32
    lr = Learner(kind="conv", precision="exact", seed=5, lr=1e-3, double_q=True, loss="huber", huber_delta=10)
    assert lr.fast is None
    sd0 = {k: v.cpu().clone() for k, v in lr.online.state_dict().items()}
    params = {k: torch.nn.Parameter(v.clone()) for k, v in sd0.items()}
    tgt = {k: v.clone() for k, v in sd0.items()}
    opt = torch.optim.Adam(params.values(), lr=1e-3)
    for it in range(2):
        if it > 0:
            lr.online.load_state_dict({k: p.detach() for k, p in params.items()})
            for key, buf in (("exp_avg", lr.m), ("exp_avg_sq", lr.v)):
                buf.copy_(torch.cat([opt.state[p][key].reshape(-1) for p in params.values()]).cuda())
        g = torch.Generator().manual_seed(10 + it)
        x = (torch.rand(B, 11, 11, 6, generator=g) < 0.3).float()
        x[..., 2] = torch.rand(B, 11, 11, generator=g) * 0.8
        x2 = (torch.rand(B, 11, 11, 6, generator=g) < 0.3).float()
        a = torch.randint(0, 5, (B,), generator=g, dtype=torch.int32)
        r = torch.randn(B, generator=g) * 30
        d = (torch.rand(B, generator=g) < 0.2).to(torch.uint8)
        m1, m2, m3 = ((torch.rand(B, 512, generator=g) >= 0.2).to(torch.uint8) for _ in range(3))
        loss = lr.learn(x.cuda(), a.cuda(), r.cuda(), d.cuda(), x2.cuda(), m1.cuda(), m2.cuda(),
                        mask_select=m3.cuda())
        sel = lr.last_sel.cpu()
        with torch.no_grad():
            # B = 32: one differing row is 3 %, so only the near-tie rule is applied here
            _check_selection(sel, _conv_forward(params, x2, m3), 0.0)
            y = r + 0.99 * _conv_forward(tgt, x2, m2).gather(1, sel.long().unsqueeze(1)).squeeze(1) * (~d.bool())
        q = _conv_forward(params, x, m1).gather(1, a.long().unsqueeze(1)).squeeze(1)
        ref_loss = F.huber_loss(q, y, delta=10.0)
        opt.zero_grad()
        ref_loss.backward()
        gnorm = torch.nn.utils.clip_grad_norm_(params.values(), 1.0)
        grads_ref = {k: p.grad.clone() for k, p in params.items()}
        opt.step()
        assert abs(loss.item() - ref_loss.item()) <= 2e-4 * abs(ref_loss.item()) + 1e-5
        assert abs(lr.norm.item() - gnorm.item()) <= 2e-4 * gnorm.item() + 1e-6
        for k in params:
            torch.testing.assert_close(lr.grads[k].cpu(), grads_ref[k], rtol=2e-3, atol=2e-6)
            diff = (lr.online[k].cpu() - params[k].detach()).abs()
            assert (diff > 1e-5).float().mean().item() <= 1e-4, (k, diff.max().item())
            assert diff.max().item() <= 1e-3, (k, diff.max().item())


# ------------------------------------------------------------------ 9. the table path
def test_selection_on_the_table_path_at_its_smallest_batch():
    """B = 8192 rows (E = 2048, R = 4 of the small env), act tables on both nets, hash dropout:
    the selection is the first-maximum argmax of the 64-row act kernel's Q on s' under the same
    dropout key (seed, drop_stream + 2), and the step's loss is the numpy restatement's from the
    device's own Q, Qt and selection."""
    _need_gpu()
    from evacx.qnet import DROPOUT_P, Learner
    lay, env = _env_obs(E=2048, steps=4)
    B, c = 8192, lay.c
    assert env.E * lay.R == B
    lr = Learner(kind="mlp", precision="f32", seed=13, double_q=True)
    for f in (lr.fast, lr.fast_t):
        f.attach_static(c, int(c.L), int(c.W), int(c.t_max))
    g = torch.Generator().manual_seed(4)
    obs = env.obs.view(-1, 8)
    s_obs = obs[torch.randperm(B, generator=g).to(DEV)].contiguous()
    s2_obs = obs[torch.randperm(B, generator=g).to(DEV)].contiguous()
    s2_obs[:3 * B // 4, 6] = int(c.t_max)  # whole tiles past the fire's last step: the table path
    s_obs, s2_obs = s_obs.view(-1), s2_obs.view(-1)
    a = torch.randint(0, 5, (B,), generator=g, dtype=torch.int32).to(DEV)
    r = (torch.randn(B, generator=g) * 30).to(DEV)
    d = (torch.rand(B, generator=g) < 0.2).to(torch.uint8).to(DEV)
    loss = lr.learn_obs(lay.c, s_obs, a, r, d, s2_obs, B, update=False)
    q = torch.empty(B, 5, device=DEV)
    lr.fast.act(lay.c, s2_obs, B, drop=(lr.seed, lr.drop_stream + 2, DROPOUT_P, None, 0), q=q, kernel64=True)
    torch.cuda.synchronize()
    assert torch.equal(lr.last_sel.long(), q.argmax(1))
    assert lr.last_sel.unique().numel() > 1
    Q = lr.net.ws.get("fq", (B * 5,), torch.float32, lr.device).view(B, 5).cpu().numpy()
    Qt = lr.net.ws.get("fqt", (B * 5,), torch.float32, lr.device).view(B, 5).cpu().numpy()
    _, _, l = np_td(Q, Qt, a.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), 0.99, B, lr.last_sel.cpu().numpy(), 0.0,
                    None)
    want = float(l.astype(np.float64).mean())
    assert abs(loss.item() - want) <= 2e-4 * abs(want), (loss.item(), want)


# ------------------------------------------------------------------ 10. soft update
def _np_polyak(tau, p, t):
    from evacx.qmlp import polyak_coeffs
    tf, omt = polyak_coeffs(tau)
    assert np.float32(tf) == np.float32(tau) and np.float32(omt) == np.float32(1 - tau)
    return np.float32(tau) * p + np.float32(1 - tau) * t


@pytest.mark.parametrize("tau", [0.005, 0.37])
def test_soft_update_blend_and_repack(small_env, tau):
    """Learner.soft_update on the x3 MLP: the target's flat buffer is np.float32(tau) * p +
    np.float32(1 - tau) * t bit for bit, every packed operand buffer equals pack3 / pack_occ3 of
    that buffer, and the attached act table equals the one rebuilt by weights_written."""
    from evacx.qnet import Learner
    lay, _ = small_env
    c = lay.c
    lr = Learner(kind="mlp", precision="f32", seed=5, target_tau=tau)
    lr.fast_t.attach_static(c, int(c.L), int(c.W), int(c.t_max))
    g = torch.Generator().manual_seed(1)
    lr.online.flat.add_((torch.randn(lr.online.numel, generator=g) * 0.05).to(DEV))
    lr.fast.repack()
    p, t = lr.online.flat.cpu().numpy(), lr.target.flat.cpu().numpy()
    packed0 = [x.clone() for x in _packed(lr.fast_t)]
    lr.soft_update()
    torch.cuda.synchronize()
    want = _np_polyak(tau, p, t)
    assert want.dtype == np.float32
    assert np.array_equal(lr.target.flat.cpu().numpy(), want)
    assert np.array_equal(lr.online.flat.cpu().numpy(), p)
    got = [x.clone() for x in _packed(lr.fast_t)]
    table = lr.fast_t._static[2].clone()
    assert any(not torch.equal(x, y) for x, y in zip(got, packed0))
    lr.weights_written(target=True)  # pack3 + pack_occ3 of the blended buffer, then the table
    torch.cuda.synchronize()
    for name, x, y in zip(PACKED, got, _packed(lr.fast_t)):
        assert torch.equal(x, y), name
    assert torch.equal(table, lr.fast_t._static[2])


PACKED = ("w1b", "w1l", "b1c", "w2b", "w2l", "w2t", "w2tl", "w1o", "w1ol")


def _packed(fast):
    return [getattr(fast, n) for n in PACKED]


def test_soft_update_without_the_fused_mlp_and_evx_polyak_alone():
    _need_gpu()
    from evacx.qmlp import polyak_coeffs
    from evacx._lib import check, lib
    from evacx.qnet import Learner
    lr = Learner(kind="mlp", precision="exact", seed=5, target_tau=0.37)
    assert lr.fast_t is None
    lr.online.flat.mul_(1.25)
    p, t = lr.online.flat.cpu().numpy(), lr.target.flat.cpu().numpy()
    lr.soft_update()
    assert np.array_equal(lr.target.flat.cpu().numpy(), _np_polyak(0.37, p, t))
    n = 1_000_003
    g = torch.Generator().manual_seed(2)
    pp = torch.randn(n + 5, generator=g).to(DEV)
    tt = torch.randn(n + 5, generator=g).to(DEV)
    pn, tn = pp.cpu().numpy(), tt.cpu().numpy()
    tf, omt = polyak_coeffs(0.005)
    check(lib().evx_polyak(pp.data_ptr(), tt.data_ptr(), n, tf, omt, None), "polyak")
    torch.cuda.synchronize()
    out = tt.cpu().numpy()
    assert np.array_equal(out[:n], _np_polyak(0.005, pn[:n], tn[:n]))
    assert np.array_equal(out[n:], tn[n:])  # nothing past n


# ------------------------------------------------------------------ 11. the trainer
def _trainer(lay, steps, **kw):
    from evacx.trainer import VecTrainer
    tr = VecTrainer(lay, 64, batch=256, replay_capacity=4096, target_every=5, lr=1e-3, **kw)
    t0 = tr.learner.target.flat.clone()
    for _ in range(steps):
        tr.step()
    tr.sync()
    torch.cuda.synchronize()
    tr.env.check_err()
    return tr, t0


ON = dict(double_q=True, loss="huber", huber_delta=10, target_tau=0.01)


@pytest.fixture(scope="module")
def trainer_layout():
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    return DeviceLayout(build_tables(synthetic(64, 64, 4)), 300)


@pytest.mark.parametrize("lagged,replay", [(False, "uniform"), (False, "prioritized"), (True, "uniform")])
def test_trainer_with_options(trainer_layout, lagged, replay):
    lay = trainer_layout
    sched = dict(lagged_learn=lagged, replay=replay)
    a, t0 = _trainer(lay, 30, **sched, **ON)
    b, _ = _trainer(lay, 30, **sched, **ON)
    off, _ = _trainer(lay, 30, **sched)
    assert a.learn_steps >= 29 and torch.isfinite(a.last_loss).all()
    assert a.learner.last_sel is not None and a.learner.last_sel.numel() == 256
    assert int(a.learner.last_sel.min()) >= 0 and int(a.learner.last_sel.max()) <= 4
    la, lb = a.learner, b.learner
    assert torch.equal(la.online.flat, lb.online.flat) and torch.equal(la.target.flat, lb.target.flat)
    assert torch.isfinite(la.online.flat).all() and torch.isfinite(la.target.flat).all()
    assert not torch.equal(la.online.flat, off.learner.online.flat)
    assert not torch.equal(la.target.flat, la.online.flat)  # never hard-copied
    assert not torch.equal(la.target.flat, t0)              # but moved


def test_trainer_options_at_their_defaults_change_nothing(trainer_layout):
    lay = trainer_layout
    a, _ = _trainer(lay, 20)
    b, _ = _trainer(lay, 20, double_q=False, loss="mse", huber_delta=1.0, target_tau=0.0)
    for x, y in ((a.learner.online.flat, b.learner.online.flat), (a.learner.target.flat, b.learner.target.flat),
                 (a.learner.m, b.learner.m), (a.learner.v, b.learner.v), (a.last_loss, b.last_loss),
                 (a.actions, b.actions), (a.env.obs, b.env.obs)):
        assert torch.equal(x, y)
    assert a.learner.drop_stream == b.learner.drop_stream and b.learner.last_sel is None


@pytest.mark.parametrize("nets", ["per_robot", "qmix"])
@pytest.mark.parametrize("opt", [dict(double_q=True), dict(loss="huber"), dict(huber_delta=2.0),
                                 dict(target_tau=0.01)])
def test_trainer_grouped_nets_refuse_the_options(trainer_layout, nets, opt):
    from evacx.trainer import VecTrainer
    with pytest.raises(ValueError, match="nets='shared'"):
        VecTrainer(trainer_layout, 64, batch=256, replay_capacity=4096, nets=nets, **opt)


# ------------------------------------------------------------------ 12. the drop-in agent
def test_dropin_agent_reads_the_option_keys():
    _need_gpu()
    from Louvre_Evacuation.agents.dqn_agent import DQNAgent
    base = {"batch_size": 32, "warmup_steps": 0, "seed": 3}
    ag = DQNAgent((11, 11, 6), 5, torch.device("cuda"), dict(base, double_dqn=True, loss="huber", huber_delta=10.0))
    lr = ag._learner
    assert (lr.double_q, lr.loss_kind, lr.huber_delta, lr.target_tau) == (True, "huber", 10.0, 0.0)
    rng = np.random.RandomState(0)
    for _ in range(40):
        s = rng.rand(11, 11, 6)
        ag.remember(s, int(rng.randint(5)), float(rng.randn() * 30), rng.rand(11, 11, 6), bool(rng.rand() < 0.2))
    loss = ag.learn()
    assert loss is not None and np.isfinite(loss)
    assert lr.last_sel is not None and lr.last_sel.numel() == 32
    plain = DQNAgent((11, 11, 6), 5, torch.device("cuda"), base)._learner
    assert (plain.double_q, plain.loss_kind, plain.huber_delta, plain.target_tau) == (False, "mse", 1.0, 0.0)
    with pytest.raises(ValueError):
        DQNAgent((11, 11, 6), 5, torch.device("cuda"), dict(base, loss="l1"))
