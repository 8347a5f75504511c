"""Double-Q, Huber, Polyak and n-step returns for per-robot and QMIX nets on the GPU: GroupedQMix
with every option against torch float64 autograd, and MultiAgentTrainer(nets="per_robot" / "qmix") with
them -- the learn step against GroupedLearner.learn_obs by hand, the sampled n-step rows against the
numpy restatement (tests/marl_opts_util.py), the target mixer's blend, and the defaults bit for bit."""
import numpy as np
import pytest
import torch

import learn_util as lu
import marl_opts_util as mu
from test_qgroup_gpu import OPERANDS, _need_gpu
from test_td_options_gpu import _np_polyak

pytestmark = pytest.mark.gpu

R, E = 4, 64
OPTS = dict(double_q=True, loss="huber", huber_delta=15.0, target_tau=0.25, n_step=3)


@pytest.fixture(scope="module")
def layout():
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    return DeviceLayout(build_tables(synthetic(48, 48, R)), 300)


def _trainer(lay, nets, steps, plain=False, **kw):
    from evacx.trainer import MultiAgentTrainer, VecTrainer
    cls = VecTrainer if plain else MultiAgentTrainer
    tr = cls(lay, E, batch=8 * R * 2, replay_capacity=1 << 12, nets=nets, epsilon=0.3, learner_seed=3, lr=1e-3,
                    **kw)
    for _ in range(steps):
        tr.step()
    tr.sync()
    torch.cuda.synchronize()
    return tr


# ------------------------------------------------------------------ GroupedQMix against float64
@pytest.mark.parametrize("n", [2, 16])
def test_grouped_qmix_step_with_options_matches_float64(n):
    """One GroupedQMix step with double_q, the Huber loss and a discount per joint row, dropout off,
    B = 64, against the agents, both mixers and the loss in float64 under one autograd backward, the
    bootstrap actions taken from the device (last_sel); then clip_grad_norm_(1.0) + Adam per agent and
    for the mixer. The bars of test_grouped_qmix_step_at_16_agents_matches_float64: loss rtol 2e-4
    (+1e-5); per-agent norm rtol 2e-4 (+1e-6); clipped gradients: at most 1e-4 of the elements beyond
    rtol 2e-3 + 1e-5 max |grad|, none beyond 1e-3 max |grad|; parameters: at most 1e-3 of the elements
    beyond 1e-5, none beyond 2e-3; mixer norm rtol 2e-4 (+1e-6), mixer parameters rtol 1e-4, atol 1e-5.

    Separately last_sel is the float64 argmax of the online nets at s2 on every row whose top-two gap
    exceeds 1e-3 max |Q| (the x3 forward is f32-accurate: a closer pair may order either way); at
    most 5 % of the rows are that close, judged on the float64 values alone."""
    _need_gpu()
    from evacx.qgroup import GroupedLearner, GroupedQMix
    from evacx.qmix import MixingNetwork
    B = 64
    lay, env = lu.small_env(4096)
    grp = GroupedLearner(n, seed=70, lr=1e-3)
    grp.drop_p = 0.0
    for j in range(n):
        grp.target[j].init_like_torch(2070 + j)
    grp.fast_t.repack()
    torch.manual_seed(5)
    mixing = MixingNetwork(n)
    with torch.no_grad():
        mixing.fc1_bias.normal_()
        mixing.fc2_bias.normal_()
    qm = GroupedQMix(grp, mixing=mixing.cuda())
    qm.mix_t.copy_(torch.randn(qm.nmix))  # a target mixer of its own
    gen = torch.Generator().manual_seed(6)
    gb = lu.grouped_batch(env, n, B, gen)
    r = (torch.randn(B, generator=gen) * 30).cuda()
    d = (torch.rand(B, generator=gen) < 0.2).to(torch.uint8).cuda()
    grow = (0.99 ** torch.randint(1, 4, (B,), generator=gen).float()).cuda()
    delta = 15.0
    dev, ref = mu.qmix_opt_step_and_references(qm, lay, env, gb, r, d, delta, grow)
    print(f"n={n}: loss {dev.loss:.9g} ref {ref.loss:.9g}; {ref.within} of {B} rows within delta; mixer norm "
          f"{dev.mix_norm:.9g} ref {ref.mix_norm:.9g}")
    assert 0 < ref.within < B, "the Huber loss has one branch only on these inputs"
    assert abs(dev.loss - ref.loss) <= 2e-4 * abs(ref.loss) + 1e-5, (dev.loss, ref.loss)
    for j, (dj, rj) in enumerate(zip(dev.agents, ref.agents)):
        gd = torch.cat([t.reshape(-1) for t in dj.grads.values()]).double()
        gr = torch.cat([t.reshape(-1) for t in rj.grads.values()])
        gs = gr.abs().max().item()
        err = (gd - gr).abs()
        bad = (err > 2e-3 * gr.abs() + 1e-5 * gs).double().mean().item()
        pd = torch.cat([t.reshape(-1) for t in dj.params.values()]).double()
        diff = (pd - torch.cat([t.reshape(-1) for t in rj.params.values()])).abs()
        print(f"agent {j}: norm {dj.norm:.9g} ref {rj.norm:.9g}; grads beyond the bar {bad:.2e}, max err "
              f"{err.max().item():.3e} of max |grad| {gs:.3e}; params beyond 1e-5 "
              f"{(diff > 1e-5).double().mean().item():.2e}, max {diff.max().item():.3e}")
        assert abs(dj.norm - rj.norm) <= 2e-4 * rj.norm + 1e-6, (j, dj.norm, rj.norm)
        assert bad <= 1e-4 and err.max().item() <= 1e-3 * gs, (j, bad, err.max().item(), gs)
        assert (diff > 1e-5).double().mean().item() <= 1e-3 and diff.max().item() <= 2e-3, j
    assert abs(dev.mix_norm - ref.mix_norm) <= 2e-4 * ref.mix_norm + 1e-6, (dev.mix_norm, ref.mix_norm)
    torch.testing.assert_close(dev.mix.double(), ref.mix, rtol=1e-4, atol=1e-5)
    # the bootstrap actions themselves
    top2 = ref.q2.topk(2, dim=2)[0]
    clear = (top2[..., 0] - top2[..., 1]) > 1e-3 * ref.q2.abs().max()
    close = 1.0 - clear.double().mean().item()
    print(f"n={n}: {close:.2%} of the rows have a top-two gap within 1e-3 max |Q|")
    assert close <= 0.05
    assert torch.equal(dev.sel[clear], ref.q2.argmax(2)[clear])


# ------------------------------------------------------------------ VecTrainer, per-robot nets
def test_per_robot_learn_step_with_options_equals_learn_obs_by_hand(layout):
    """MultiAgentTrainer(nets="per_robot") with every option: its learn step -- the fused n-step sampler, then
    the grouped learn step and soft update -- equals GroupedLearner.learn_obs and soft_update called by
    hand on a copy of the nets with the same sampled rows and options, bit for bit."""
    from evacx.qgroup import GroupedLearner
    lay = layout
    tr = _trainer(lay, "per_robot", 5, **OPTS)
    gl = tr.glearner
    assert tr.last_loss is not None and torch.isfinite(tr.last_loss).all() and gl.last_sel is not None
    assert "gamma_row" in tr.samp and int(tr.samp["nlen"].max()) > 1
    ref = GroupedLearner(R, "cuda", lr=gl.lr, gamma=gl.gamma, seed=gl.seed)
    for name in ("flat", "tflat", "m", "v"):
        getattr(ref, name).copy_(getattr(gl, name))
    for k in OPERANDS:
        ref.fast.bufs[k].copy_(gl.fast.bufs[k])
        ref.fast_t.bufs[k].copy_(gl.fast_t.bufs[k])
    ref.adam_step, ref.drop_stream = gl.adam_step, gl.drop_stream
    steps = tr.learn_steps
    loss = tr.learn().clone()
    torch.cuda.synchronize()
    assert tr.learn_steps == steps + 1 and tr.last_range == tr.replay.live_range()
    sp, Bn = tr.samp, tr.batch // R
    ring = mu.host_ring(tr.replay)
    want = mu.np_sample_nstep_agents(ring, Bn, R, 0, tr.seed + 1, steps * tr.batch, tr.last_range[0], tr.last_range[1],
                                     E * R, 3, gl.gamma)
    for k, dk in (("s", "s"), ("a", "a"), ("s2", "s2"), ("r", "r"), ("done", "done"), ("gamma_row", "gamma_row"),
                  ("len", "nlen"), ("idx", "idx")):
        assert np.array_equal(sp[dk].cpu().numpy().reshape(-1), np.ascontiguousarray(want[k]).reshape(-1)), k
    loss_ref = ref.learn_obs(lay.c, sp["s"], sp["a"], sp["r"], sp["done"], sp["s2"], Bn, gamma_row=sp["gamma_row"],
                             double_q=True, huber_delta=[15.0] * R).clone()
    ref.soft_update([0.25] * R)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss_ref) and torch.equal(gl.last_sel, ref.last_sel)
    for name in ("flat", "tflat", "m", "v", "gflat", "norm"):
        assert torch.equal(getattr(gl, name), getattr(ref, name)), name
    for k in OPERANDS:
        assert torch.equal(gl.fast.bufs[k], ref.fast.bufs[k]), k
        assert torch.equal(gl.fast_t.bufs[k], ref.fast_t.bufs[k]), ("target", k)
    assert not torch.equal(gl.tflat, gl.flat)  # a blend, not a copy


# ------------------------------------------------------------------ VecTrainer, QMIX nets
def test_qmix_trainer_with_options(layout):
    """MultiAgentTrainer(nets="qmix", double_q, Huber, target_tau = 0.25, n_step = 3), 8 steps: finite
    losses, every agent and the mixer move, chains longer than one slot; one more learn step by hand:
    its sampled s / a / r / done / s2 / gamma_row / len / idx equal the numpy restatement on the
    ring's arrays read back from the device, and the target mixer becomes the blend of its previous
    value and the new mixer, bit for bit (as the evx_polyak test compares)."""
    lay = layout
    tr = _trainer(lay, "qmix", 0, target_every=3, **OPTS)
    p0, m0 = tr.glearner.flat.clone(), tr.qmix.mix.clone()
    losses = []
    for _ in range(8):
        tr.step()
        losses.append(tr.last_loss.clone())
    tr.sync()
    torch.cuda.synchronize()
    assert len(losses) == 8 and all(torch.isfinite(x).all() for x in losses)
    assert bool((tr.glearner.flat != p0).any(dim=1).all()) and not torch.equal(tr.qmix.mix, m0)
    assert int(tr.samp["nlen"].max()) > 1 and tr.glearner.last_sel is not None
    assert tr.glearner.drop_stream == 3 * tr.learn_steps
    mt0, t0 = tr.qmix.mix_t.cpu().numpy(), tr.glearner.tflat.clone()
    steps = tr.learn_steps
    assert torch.isfinite(tr.learn()).all()
    torch.cuda.synchronize()
    sp, Bn = tr.samp, tr.batch // R
    ring = mu.host_ring(tr.replay)
    want = mu.np_sample_nstep_agents(ring, Bn, R, 1, tr.seed + 1, steps * tr.batch, tr.last_range[0], tr.last_range[1],
                                     E * R, 3, tr.glearner.gamma)
    assert tr.last_range == ring.live_range()
    for k, dk in (("s", "s"), ("a", "a"), ("s2", "s2"), ("r", "r"), ("done", "done"), ("gamma_row", "gamma_row"),
                  ("len", "nlen"), ("idx", "idx")):
        assert np.array_equal(sp[dk].cpu().numpy().reshape(-1), np.ascontiguousarray(want[k]).reshape(-1)), k
    assert (want["len"] > 1).any()
    # agent 0's rows are the joint rows': every agent's r / done / gamma_row / len repeat them
    for dk in ("r", "done", "gamma_row", "nlen"):
        rows = sp[dk].view(R, Bn)
        assert bool((rows == rows[0]).all()), dk
    assert np.array_equal(tr.qmix.mix_t.cpu().numpy(), _np_polyak(0.25, tr.qmix.mix.cpu().numpy(), mt0))
    assert not torch.equal(tr.glearner.tflat, t0) and not torch.equal(tr.glearner.tflat, tr.glearner.flat)


# ------------------------------------------------------------------ defaults, and every option alone
@pytest.mark.parametrize("nets", ["per_robot", "qmix"])
def test_options_at_their_defaults_change_nothing(layout, nets):
    a = _trainer(layout, nets, 6, plain=True, target_every=2)  # a VecTrainer built without naming the options
    b = _trainer(layout, nets, 6, target_every=2, double_q=False, loss="mse", huber_delta=1.0, target_tau=0.0, n_step=1)
    pairs = [(a.actions, b.actions), (a.last_loss, b.last_loss), (a.env.obs, b.env.obs)]
    pairs += [(getattr(a.glearner, k), getattr(b.glearner, k)) for k in ("flat", "tflat", "m", "v")]
    if nets == "qmix":
        pairs += [(getattr(a.qmix, k), getattr(b.qmix, k)) for k in ("mix", "mix_t", "mix_m", "mix_v")]
    for x, y in pairs:
        assert torch.equal(x, y)
    assert a.glearner.drop_stream == b.glearner.drop_stream == 2 * b.learn_steps
    assert b.glearner.last_sel is None and "gamma_row" not in b.samp and "idx" not in b.samp and b.last_range is None


@pytest.mark.parametrize("nets", ["per_robot", "qmix"])
@pytest.mark.parametrize("opt", [dict(double_q=True), dict(loss="huber"), dict(huber_delta=2.0),
                                 dict(target_tau=0.01)])
def test_trainer_grouped_nets_take_the_options(layout, nets, opt):
    """Each option VecTrainer refuses for the grouped nets, alone, through MultiAgentTrainer: it is built, trains, and the
    option shows -- Double-Q's actions, a target that is neither its start nor a copy, a Huber loss
    that differs from the squared error (huber_delta without loss='huber' changes nothing)."""
    plain = _trainer(layout, nets, 4)
    tr = _trainer(layout, nets, 4, **opt)
    gl = tr.glearner
    assert tr.last_loss is not None and torch.isfinite(tr.last_loss).all()
    assert (gl.last_sel is not None) == ("double_q" in opt)
    same = torch.equal(gl.flat, plain.glearner.flat)
    if "target_tau" in opt:
        assert not torch.equal(gl.tflat, plain.glearner.tflat) and not torch.equal(gl.tflat, gl.flat)
        if nets == "qmix":
            assert not torch.equal(tr.qmix.mix_t, plain.qmix.mix_t) and not torch.equal(tr.qmix.mix_t, tr.qmix.mix)
    elif "huber_delta" in opt:
        assert same and torch.equal(tr.last_loss, plain.last_loss)
    else:
        assert not same


# ------------------------------------------------------------------ the runner
@pytest.mark.parametrize("nets,robots", [("per_robot", 2), ("qmix", 2), ("qmix", 3)])
def test_train_vec_trains_and_saves_per_robot_and_qmix_nets(tmp_path, capsys, nets, robots):
    """train_vec --robots 2 | 3 --nets per_robot | qmix with every option flag (3 robots: a ring that
    is no power of two): the start line names the mode, agent<r>.pth hold the reference's checkpoint dict and load through evaluate_vec's loader
    with the trained weights, QMIX adds mixer.pth, and --eval-episodes evaluates the per-robot policy."""
    _need_gpu()
    from Louvre_Evacuation.runners import evaluate_vec as ev
    from Louvre_Evacuation.runners import train_vec as tv
    cfg = tmp_path / "small.yaml"
    cfg.write_text("env:\n  width: 36\n  height: 30\n  fire_zones: [[18, 14]]\n  exit_location: [36, 15]\n"
                   "  num_people: 40\nagent:\n  gamma: 0.99\n  epsilon: 1.0\n  epsilon_min: 0.02\n"
                   "  epsilon_decay: 0.9995\n  learning_rate: 0.0001\n  batch_size: 32\n  target_update_freq: 20\n"
                   "  memory_size: 4096\n  target_tau: 0.05\nsave_path: \"unused\"\n")
    out = tmp_path / "out"
    tr = tv.train_vec(tv.parse_args(["--config", str(cfg), "--envs", "32", "--steps", "12", "--log-every", "6",
                                     "--robots", str(robots), "--nets", nets, "--out", str(out), "--double-q",
                                     "--loss", "huber", "--huber-delta", "10", "--n-step", "2", "--eval-episodes", "1", "--eval-envs", "8"]))
    text = capsys.readouterr().out
    assert f"{nets} nets" in text and f"{robots} robots" in text and "double-Q target" in text and "n_step 2" in text
    assert "soft tau 0.05" in text and "greedy evaluation over 8 episodes" in text
    assert tr.per_robot and tr.n_step == 2 and tr.target_tau == 0.05 and tr.learn_steps > 0
    assert (tr.qmix is not None) == (nets == "qmix") and tr.glearner.last_sel is not None
    assert tr.replay.capacity % robots == 0 and tr.batch % (2 * robots) == 0
    for g in range(robots):
        ck = torch.load(out / f"agent{g}.pth", map_location="cpu", weights_only=True)
        assert set(ck) == {"q_network", "target_network", "optimizer", "epsilon", "steps"}
        assert list(ck["q_network"]) == list(tr.glearner.state_dict(g))
        assert ck["steps"] == tr.learn_steps and len(ck["optimizer"]["state"]) == 6
        lr = ev.load_learner(str(out / f"agent{g}.pth"), "cuda")
        assert torch.equal(lr.online.flat, tr.glearner.flat[g])
    assert not (out / "dqn_model.pth").exists()
    assert (out / "mixer.pth").exists() == (nets == "qmix")
    if nets == "qmix":
        mk = torch.load(out / "mixer.pth", map_location="cpu", weights_only=True)
        flat = torch.cat([v.reshape(-1) for v in mk["mixing_network"].values()])
        assert list(mk["mixing_network"]) == ["fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias"]
        assert torch.equal(flat, tr.qmix.mix.cpu())
        assert torch.equal(torch.cat([v.reshape(-1) for v in mk["target_mixing_network"].values()]), tr.qmix.mix_t.cpu())
