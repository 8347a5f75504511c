"""n-step returns from the replay ring on the GPU: evx_replay_nstep, the per-row discount of the
two TD kernels (evx_td_opts.gamma_row), Learner(gamma_row=) and VecTrainer(n_step=).

The gather is compared bit for bit with the numpy restatement of tests/test_nstep_cpu.py
(np.float32 scalars in the kernel's stated loop order); the TD step with a per-row discount
against numpy float32 in the kernel's order of operations and torch autograd in fp32, within the
bars tests/test_td_options_gpu.py states for the same kernels."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_nstep_cpu import CAP, NSTEPS, RANGES, STRIDE, np_nstep, range_slots, ring_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda"
GAMMA = 0.99


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ring(r, done, s2, s=None, a=None):
    """A Replay whose tensors are filled directly from host arrays."""
    from evacx.trainer import Replay
    rp = Replay(len(r), DEV)
    rp.r.copy_(torch.from_numpy(r))
    rp.done.copy_(torch.from_numpy(done))
    rp.s2.copy_(torch.from_numpy(s2.reshape(-1)))
    if s is not None:
        rp.s.copy_(torch.from_numpy(s.reshape(-1)))
    if a is not None:
        rp.a.copy_(torch.from_numpy(a))
    return rp


def _out(B, idx=False):
    o = dict(s=torch.full((B * 8,), -1, dtype=torch.int32, device=DEV),
             s2=torch.full((B * 8,), -1, dtype=torch.int32, device=DEV),
             a=torch.full((B,), -1, dtype=torch.int32, device=DEV),
             r=torch.full((B,), float("nan"), device=DEV),
             done=torch.full((B,), 7, dtype=torch.uint8, device=DEV),
             gamma_row=torch.full((B,), float("nan"), device=DEV),
             nlen=torch.full((B,), -1, dtype=torch.int32, device=DEV))
    if idx:
        o["idx"] = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    return o


def _assert_rows(out, ref, B):
    R, G, D, S2, L = ref
    torch.cuda.synchronize()
    assert torch.equal(out["r"][:B].cpu(), torch.from_numpy(R))
    assert torch.equal(out["gamma_row"][:B].cpu(), torch.from_numpy(G))
    assert torch.equal(out["done"][:B].cpu(), torch.from_numpy(D))
    assert torch.equal(out["nlen"][:B].cpu(), torch.from_numpy(L))
    assert torch.equal(out["s2"][:B * 8].cpu().view(B, 8), torch.from_numpy(S2))


# ------------------------------------------------------------------ 1. the kernel
@pytest.fixture(scope="module")
def kernel_ring():
    _need_gpu()
    r, done, s2 = ring_fixture()
    return (r, done, s2), _ring(r, done, s2)


@pytest.mark.parametrize("base,count", RANGES)
def test_replay_nstep_matches_the_restatement_bit_for_bit(kernel_ring, base, count):
    """Capacity 64, stride 8, every slot of the range (B = count), then 300 repeated indices (more
    than one 256-thread block, a ragged tail); n_step 1, 2, 3, 5."""
    (r, done, s2), rp = kernel_ring
    rng = np.random.RandomState(count)
    for idx in (range_slots(base, count), range_slots(base, count)[rng.randint(0, count, 300)]):
        B = len(idx)
        didx = torch.from_numpy(idx).to(DEV)
        for n in NSTEPS:
            out = _out(B + 3)
            rp.nstep(didx, B, base, count, STRIDE, n, GAMMA, out)
            _assert_rows(out, np_nstep(r, done, s2, idx, base, count, STRIDE, n, GAMMA), B)
            for k in ("r", "gamma_row"):  # nothing past B
                assert torch.isnan(out[k][B:]).all()
            assert (out["nlen"][B:] == -1).all() and (out["s2"][B * 8:] == -1).all() and (out["done"][B:] == 7).all()
    # len is optional
    out = _out(count)
    del out["nlen"]
    rp.nstep(torch.from_numpy(range_slots(base, count)).to(DEV), count, base, count, STRIDE, 3, GAMMA, out)
    torch.cuda.synchronize()
    assert torch.equal(out["r"].cpu(), torch.from_numpy(np_nstep(r, done, s2, range_slots(base, count), base, count,
                                                                 STRIDE, 3, GAMMA)[0]))


def test_replay_nstep_keeps_a_slot_outside_the_range(kernel_ring):
    """A slot with d0 >= count keeps its own row (L = 1) and no successor is read; a stride beyond
    the ring finds no successor either."""
    (r, done, s2), rp = kernel_ring
    idx = np.array([50, 63, 41, 3], np.int64)
    out = _out(4)
    rp.nstep(torch.from_numpy(idx).to(DEV), 4, 0, 40, STRIDE, 3, GAMMA, out)
    ref = np_nstep(r, done, s2, idx, 0, 40, STRIDE, 3, GAMMA)
    assert (ref[4][:3] == 1).all()
    _assert_rows(out, ref, 4)
    out = _out(4)
    rp.nstep(torch.from_numpy(idx).to(DEV), 4, 0, 40, 1 << 40, 3, GAMMA, out)
    torch.cuda.synchronize()
    assert (out["nlen"] == 1).all() and torch.equal(out["r"].cpu(), torch.from_numpy(r[idx]))


# ------------------------------------------------------------------ 2. n_step = 1 is the identity
def _run_td(Q, Qt, act, rew, done, B, nets, w, sel, delta, gamma_row, use_opt=True):
    from evacx.qmlp import td_opts
    from evacx._lib import check, lib
    L = lib()
    A = Q.shape[1]
    dQ = torch.full((nets * B, A), float("nan"), device=DEV)
    loss = torch.full((nets,), float("nan"), device=DEV)
    td_abs = torch.full((nets * B,), float("nan"), device=DEV)
    ws = torch.zeros(int(L.evx_td_loss_ws_floats(B, nets)), device=DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    o = td_opts(sel, delta, gamma_row)
    check(L.evx_td_loss_opt(p(Q), p(Qt), A, p(act), p(rew), p(done), GAMMA, B, nets, p(w), p(dQ), p(loss), p(td_abs),
                            None, 0, p(ws), ws.numel(), C.byref(o) if use_opt else None, None), "td_loss_opt")
    torch.cuda.synchronize()
    return dQ, loss, td_abs


def _td_inputs(B, nets, seed):
    g = torch.Generator().manual_seed(seed)
    n, A = nets * B, 5
    Q = (torch.randn(n, A, generator=g) * 3).to(DEV)
    Qt = (torch.randn(n, A, generator=g) * 3).to(DEV)
    act = torch.randint(0, A, (n,), generator=g, dtype=torch.int32).to(DEV)
    rew = (torch.randn(n, generator=g) * 30).to(DEV)
    done = (torch.rand(n, generator=g) < 0.2).to(torch.uint8).to(DEV)
    sel = torch.randint(0, A, (n,), generator=g, dtype=torch.int32).to(DEV)
    w = (torch.rand(n, generator=g) * 0.9 + 0.1).to(DEV)
    grow = torch.rand(n, generator=g).to(DEV)
    grow[::7] = 0.0
    grow[3::11] = 1.0
    return Q, Qt, act, rew, done, sel, w, grow


def test_n_step_1_is_the_identity_of_the_sampler(kernel_ring):
    (r, done, s2), rp = kernel_ring
    rp.size, B = 40, 32
    samp = _out(B, idx=True)
    rp.sample(B, 11, 0, samp)
    torch.cuda.synchronize()
    idx = samp["idx"].cpu().numpy()
    assert len(set(idx.tolist())) == B and idx.min() >= 0 and idx.max() < 40
    assert torch.equal(samp["r"].cpu(), torch.from_numpy(r[idx]))
    out = _out(B)
    rp.nstep(samp["idx"], B, 0, 40, STRIDE, 1, GAMMA, out)
    torch.cuda.synchronize()
    for k in ("r", "done", "s2"):
        assert torch.equal(out[k], samp[k]), k
    assert (out["gamma_row"] == float(np.float32(GAMMA))).all() and (out["nlen"] == 1).all()
    # the windowed sampler writes idx too
    samp = _out(B, idx=True)
    rp.sample_window(24, 56, B, 11, 0, samp)
    out = _out(B)
    rp.nstep(samp["idx"], B, 24, 56, STRIDE, 1, GAMMA, out)
    torch.cuda.synchronize()
    d0 = (samp["idx"].cpu().numpy() - 24) % CAP
    assert (d0 < 56).all() and len(set(d0.tolist())) == B
    for k in ("r", "done", "s2"):
        assert torch.equal(out[k], samp[k]), k


@pytest.mark.parametrize("B,nets", [(250, 1), (64, 3)])
def test_gamma_row_equal_to_gamma_is_the_scalar_path_bit_for_bit(B, nets):
    _need_gpu()
    Q, Qt, act, rew, done, sel, w, _ = _td_inputs(B, nets, 7 + B)
    grow = torch.full((nets * B,), GAMMA, device=DEV)  # f32(0.99): what n_step = 1 writes
    for ss, delta, ww in ((None, 0.0, None), (sel, 10.0, w)):
        base = _run_td(Q, Qt, act, rew, done, B, nets, ww, ss, delta, None)
        got = _run_td(Q, Qt, act, rew, done, B, nets, ww, ss, delta, grow)
        for x, y in zip(got, base):
            assert torch.equal(x, y)
    null = _run_td(Q, Qt, act, rew, done, B, nets, None, None, 0.0, None, use_opt=False)
    for x, y in zip(_run_td(Q, Qt, act, rew, done, B, nets, None, None, 0.0, grow), null):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 3. a varied gamma_row
def np_td(Q, Qt, act, rew, done, grow, B, sel, delta, w):
    """include/evacx.h's per-row TD order with the row's discount, numpy float32 (every operation
    rounded to f32, no fused multiply-add); rows of one net. -> dq_at_action, |d|, l."""
    f = np.float32
    rows = np.arange(B)
    v = Qt.max(axis=1) if sel is None else Qt[rows, np.clip(sel, 0, Qt.shape[1] - 1)]
    flag = np.where(done != 0, f(0), f(1)).astype(f)
    y = rew + (grow * v) * flag
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


def _ulp_close(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)


@pytest.mark.parametrize("B,nets", [(250, 1), (64, 3)])
def test_td_loss_with_a_per_row_discount_matches_numpy_float32(B, nets):
    """evx_td_loss_opt with gamma_row in [0, 1] (0 and 1 among them) for every combination of
    sel, Huber delta and weights: dQ exactly zero off the taken action, dQ at the action and |d|
    within 1 ulp, the loss rtol 2e-4 of the float64 mean of the per-row terms."""
    _need_gpu()
    Q, Qt, act, rew, done, sel_r, w_r, grow = _td_inputs(B, nets, 100 + B)
    Qn, Qtn, an, rn, dn, gn = (t.cpu().numpy() for t in (Q, Qt, act, rew, done, grow))
    for sel in (None, sel_r):
        for delta in (0.0, 10.0):
            for w in (None, w_r):
                dQ, loss, td_abs = _run_td(Q, Qt, act, rew, done, B, nets, w, sel, delta, grow)
                dQn, tdn, lossn = dQ.cpu().numpy(), td_abs.cpu().numpy(), loss.cpu().numpy()
                for k in range(nets):
                    r0 = slice(k * B, (k + 1) * B)
                    gref, adref, lref = np_td(Qn[r0], Qtn[r0], an[r0], rn[r0], dn[r0], gn[r0], B,
                                              None if sel is None else sel.cpu().numpy()[r0], delta,
                                              None if w is None else w.cpu().numpy()[r0])
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
    # the discount matters: the scalar path gives other numbers
    assert not torch.equal(_run_td(Q, Qt, act, rew, done, B, nets, None, None, 0.0, None)[0],
                           _run_td(Q, Qt, act, rew, done, B, nets, None, None, 0.0, grow)[0])


# ------------------------------------------------------------------ 4. / 5. the learner
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


RING, RSTRIDE = 1024, 64


def _nstep_batch(env, lay, B, g, n_masks=3):
    """B n-step rows (n_step = 3) made by evx_replay_nstep from a ring of 1024 slots, 64 rows per
    step: s and s' from the env's observations, actions, rewards randn * 30, 20 % done flags, and
    explicit keep masks, all from the seeded CPU generator g. -> s_obs, s2_obs, a, R, done,
    gamma_row, masks; the chain lengths cover 1, 2 and 3."""
    from evacx.qmlp import HID
    obs = env.obs.view(-1, 8).cpu().numpy()
    n = obs.shape[0]
    s = obs[torch.randint(0, n, (RING,), generator=g).numpy()]
    s2 = obs[torch.randint(0, n, (RING,), generator=g).numpy()]
    a = torch.randint(0, 5, (RING,), generator=g, dtype=torch.int32).numpy()
    r = (torch.randn(RING, generator=g) * 30).numpy()
    d = (torch.rand(RING, generator=g) < 0.2).to(torch.uint8).numpy()
    rp = _ring(r, d, s2, s=s, a=a)
    idx = torch.randperm(RING, generator=g)[:B]
    out = _out(B)
    rp.nstep(idx.to(DEV), B, 0, RING, RSTRIDE, 3, GAMMA, out)
    ref = np_nstep(r, d, s2, idx.numpy(), 0, RING, RSTRIDE, 3, GAMMA)
    _assert_rows(out, ref, B)
    assert set(ref[4].tolist()) == {1, 2, 3}
    masks = [(torch.rand(B, HID, generator=g) >= 0.2).to(torch.uint8).to(DEV) for _ in range(n_masks)]
    di = idx.to(DEV)
    s_obs = rp.s.view(-1, 8)[di].contiguous().view(-1)
    return s_obs, out["s2"], rp.a[di].contiguous(), out["r"], out["done"], out["gamma_row"], masks


@pytest.mark.parametrize("hook", [False, True])
def test_fused_learn_chain_matches_separate_launches_with_gamma_row(small_env, hook):
    """tests/test_td_options_gpu.py::test_fused_learn_chain_matches_separate_launches_with_options
    with n-step rows: evx_qmlp_td_backward_opt's gamma_row against evx_td_loss_opt's + the separate
    backward, that test's fixture, batch and bars."""
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
            s_obs, s2_obs, a, r, d, grow, (m1, m2, m3) = _nstep_batch(env, lay, B, g)
            loss = lr.learn_obs(lay.c, s_obs, a, r, d, s2_obs, B, mask_online=m1, mask_target=m2, mask_select=m3,
                                gamma_row=grow)
        torch.cuda.synchronize()
        runs.append(dict(loss=loss.item(), norm=lr.norm.item(), sel=lr.last_sel.clone(),
                         grads={k: v.clone() for k, v in lr.grads.state_dict().items()},
                         params={k: v.clone() for k, v in lr.online.state_dict().items()}))
    sep, fus, fus2 = runs
    assert fus["loss"] == fus2["loss"] and fus["norm"] == fus2["norm"]
    for k in fus["params"]:
        assert torch.equal(fus["grads"][k], fus2["grads"][k]), k
        assert torch.equal(fus["params"][k], fus2["params"][k]), k
    assert torch.equal(sep["sel"], fus["sel"])
    assert abs(sep["loss"] - fus["loss"]) <= 1e-5 * abs(sep["loss"]) + 1e-7
    assert abs(sep["norm"] - fus["norm"]) <= 1e-5 * sep["norm"] + 1e-9
    for k in sep["params"]:
        scale = sep["grads"][k].abs().max().item()
        torch.testing.assert_close(fus["grads"][k], sep["grads"][k], rtol=1e-4, atol=1e-6 * scale + 1e-12)
        torch.testing.assert_close(fus["params"][k], sep["params"][k], rtol=1e-5, atol=2e-6)
    # the discount reaches the fused kernel: the same step without it gives another loss
    lr = Learner(kind="mlp", precision="f32", seed=33, lr=1e-3, double_q=True, loss="huber", huber_delta=10)
    g = torch.Generator().manual_seed(9)
    for it in range(3):
        s_obs, s2_obs, a, r, d, grow, (m1, m2, m3) = _nstep_batch(env, lay, B, g)
        loss = lr.learn_obs(lay.c, s_obs, a, r, d, s2_obs, B, mask_online=m1, mask_target=m2, mask_select=m3)
    assert loss.item() != fus["loss"]


@pytest.mark.parametrize("opts", [dict(), dict(double_q=True, loss="huber", huber_delta=10)],
                         ids=["mse", "double_q-huber"])
def test_x3_learn_steps_on_n_step_rows_match_torch_autograd(small_env, opts):
    """tests/test_td_options_gpu.py::test_x3_learn_steps_with_options_match_torch_autograd on
    n-step rows: y = R + gamma_row * Q_target(s2, j*) * !done, with the max target and the MSE,
    and with Double-Q + Huber (the reference takes the device's own selection); that test's bars."""
    from evacx.qmlp import K1
    from evacx.qnet import Learner
    lay, env = small_env
    B = 256
    lr = Learner(kind="mlp", precision="f32", seed=21, lr=1e-3, **opts)
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
        s_obs, s2_obs, a, r, d, grow, (m1, m2, m3) = _nstep_batch(env, lay, B, g)
        loss = lr.learn_obs(lay.c, s_obs, a, r, d, s2_obs, B, mask_online=m1, mask_target=m2, mask_select=m3,
                            gamma_row=grow)
        X = env.expand_obs(torch.float32, s_obs).reshape(B, K1)
        X2 = env.expand_obs(torch.float32, s2_obs).reshape(B, K1)
        with torch.no_grad():
            qt = torch_q(tgt, X2, m2)
            if opts:
                v = qt.gather(1, lr.last_sel.long().unsqueeze(1)).squeeze(1)
            else:
                v = qt.max(1)[0]
            y = r + grow * v * (~d.bool())
        q = torch_q(params, X, m1).gather(1, a.long().unsqueeze(1)).squeeze(1)
        ref_loss = F.huber_loss(q, y, delta=10.0) if opts else F.mse_loss(q, y)
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


def test_dense_learn_on_n_step_rows_matches_torch_autograd():
    """Learner.learn (conv net, exact f32 GEMMs, td_loss_kernel), B = 32, one step with a
    per-row discount gamma^L (f32 products, L in 1..3) against torch autograd on the CPU: the bars
    of tests/test_td_options_gpu.py::test_dense_learn_with_options_matches_torch_autograd."""
    _need_gpu()
    from evacx.qnet import Learner
    B = 32
    lr = Learner(kind="conv", precision="exact", seed=5, lr=1e-3)
    assert lr.fast is None
    params = {k: torch.nn.Parameter(v.cpu().clone()) for k, v in lr.online.state_dict().items()}
    tgt = {k: v.detach().clone() for k, v in params.items()}
    opt = torch.optim.Adam(params.values(), lr=1e-3)
    g = torch.Generator().manual_seed(10)
    x = (torch.rand(B, 11, 11, 6, generator=g) < 0.3).float()
    x[..., 2] = torch.rand(B, 11, 11, generator=g) * 0.8
    x2 = (torch.rand(B, 11, 11, 6, generator=g) < 0.3).float()
    a = torch.randint(0, 5, (B,), generator=g, dtype=torch.int32)
    r = torch.randn(B, generator=g) * 30
    d = (torch.rand(B, generator=g) < 0.2).to(torch.uint8)
    m1, m2 = ((torch.rand(B, 512, generator=g) >= 0.2).to(torch.uint8) for _ in range(2))
    g1 = np.float32(GAMMA)
    pw = np.array([g1, g1 * g1, g1 * g1 * g1], np.float32)
    grow = torch.from_numpy(pw[torch.randint(0, 3, (B,), generator=g).numpy()])
    loss = lr.learn(x.cuda(), a.cuda(), r.cuda(), d.cuda(), x2.cuda(), m1.cuda(), m2.cuda(), gamma_row=grow.cuda())
    with torch.no_grad():
        y = r + grow * _conv_forward(tgt, x2, m2).max(1)[0] * (~d.bool())
    q = _conv_forward(params, x, m1).gather(1, a.long().unsqueeze(1)).squeeze(1)
    ref_loss = F.mse_loss(q, y)
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
    with pytest.raises(ValueError, match="gamma_row"):
        lr.learn(x.cuda(), a.cuda(), r.cuda(), d.cuda(), x2.cuda(), m1.cuda(), m2.cuda(), gamma_row=grow[:5].cuda())


# ------------------------------------------------------------------ 6. - 9. the trainer
@pytest.fixture(scope="module")
def trainer_layout():
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    return DeviceLayout(build_tables(synthetic(64, 64, 4)), 300)


def _trainer(lay, steps, **kw):
    from evacx.trainer import VecTrainer
    tr = VecTrainer(lay, 64, batch=256, replay_capacity=4096, **kw)
    for _ in range(steps):
        tr.step()
    tr.sync()
    torch.cuda.synchronize()
    tr.env.check_err()
    return tr


def _host_ring(rp):
    C_ = rp.capacity
    return dict(s=rp.s.cpu().numpy().reshape(C_, 8), s2=rp.s2.cpu().numpy().reshape(C_, 8),
                r=rp.r.cpu().numpy(), done=rp.done.cpu().numpy())


def test_the_successor_of_a_slot_is_one_push_further(trainer_layout):
    """The invariant the feature rests on (it holds without it): 64 envs x 4 robots push 256 rows
    per step into a 16-step ring; after 20 steps (wrapped) every slot j of the live range with
    done[j] == 0 whose successor lies in the range has s2[j] == s[(j + 256) mod C] word for word."""
    tr = _trainer(trainer_layout, 20, target_every=5, lr=1e-3)
    rp = tr.replay
    C_, n = rp.capacity, tr.n_agents
    assert n == 256 and rp.size == C_ and tr.t * n > C_
    base, count = (rp.pos - rp.size) % C_, rp.size
    h = _host_ring(rp)
    d = np.arange(count - n)
    j = (base + d) % C_
    live = h["done"][j] == 0
    assert live.sum() > 1000
    assert np.array_equal(h["s"][(j[live] + n) % C_], h["s2"][j[live]])
    # and the rule is not vacuous: another offset breaks it
    assert not np.array_equal(h["s"][(j[live] + n + 1) % C_], h["s2"][j[live]])


@pytest.mark.parametrize("lagged,replay", [(False, "uniform"), (False, "prioritized"), (True, "uniform")])
def test_trainer_with_n_step_3(trainer_layout, lagged, replay):
    lay = trainer_layout
    kw = dict(lagged_learn=lagged, replay=replay, target_every=5, lr=1e-3)
    a = _trainer(lay, 30, n_step=3, **kw)
    b = _trainer(lay, 30, n_step=3, **kw)
    one = _trainer(lay, 30, **kw)
    assert a.learn_steps >= 28 and torch.isfinite(a.last_loss).all()
    # the last learn step's rows, recomputed from a host copy of the ring over the range it used
    # (lagged: the window; the push that ran beside it wrote outside the window only)
    h = _host_ring(a.replay)
    base, count = a.last_range
    if lagged:
        assert (base, count) != a.replay.live_range() and count == a.replay.capacity - a.n_agents
    else:
        assert (base, count) == a.replay.live_range()
    idx = a.samp["idx"].cpu().numpy()
    assert (((idx - base) % a.replay.capacity) < count).all()
    ref = np_nstep(h["r"], h["done"], h["s2"], idx, base, count, a.n_agents, 3, a.learner.gamma)
    _assert_rows(a.samp, ref, a.batch)
    assert int(a.samp["nlen"].max()) == 3 and int(a.samp["nlen"].min()) >= 1
    # the slots' own actions and observations stay the sampler's
    assert np.array_equal(a.samp["s"].cpu().numpy().reshape(-1, 8), h["s"][idx])
    la, lb = a.learner, b.learner
    assert torch.equal(la.online.flat, lb.online.flat) and torch.equal(la.target.flat, lb.target.flat)
    assert torch.isfinite(la.online.flat).all() and torch.isfinite(la.target.flat).all()
    assert not torch.equal(la.online.flat, one.learner.online.flat)
    assert "gamma_row" not in one.samp and "nlen" not in one.samp


def test_n_step_at_its_default_changes_nothing(trainer_layout):
    lay = trainer_layout
    a = _trainer(lay, 20, target_every=5, lr=1e-3)
    b = _trainer(lay, 20, target_every=5, lr=1e-3, n_step=1)
    for x, y in ((a.learner.online.flat, b.learner.online.flat), (a.learner.target.flat, b.learner.target.flat),
                 (a.learner.m, b.learner.m), (a.learner.v, b.learner.v), (a.last_loss, b.last_loss),
                 (a.actions, b.actions), (a.env.obs, b.env.obs)):
        assert torch.equal(x, y)
    assert a.learner.drop_stream == b.learner.drop_stream
    assert "idx" not in b.samp and b.last_range is None


def test_n_step_refusals(trainer_layout):
    from evacx.trainer import VecTrainer
    lay = trainer_layout
    base = dict(batch=256, replay_capacity=4096)
    with pytest.raises(ValueError, match="nets"):
        VecTrainer(lay, 64, nets="per_robot", n_step=2, **base)
    with pytest.raises(ValueError, match="nets"):
        VecTrainer(lay, 64, nets="qmix", n_step=2, **base)
    with pytest.raises(ValueError, match="groups"):
        VecTrainer(lay, 64, groups=2, n_step=2, **base)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="n_step"):
            VecTrainer(lay, 64, n_step=bad, **base)
    with pytest.raises(ValueError, match="n_step"):
        VecTrainer(lay, 64, n_step=17, **base)  # 17 * 256 > 4096: no chain could complete
    tr = VecTrainer(lay, 64, n_step=2, **base)
    with pytest.raises(ValueError, match="extra_reset"):
        tr.step(extra_reset=torch.zeros(64, dtype=torch.bool, device=DEV))
    tr.step()  # and the trainer is still usable
    tr.sync()
    torch.cuda.synchronize()
