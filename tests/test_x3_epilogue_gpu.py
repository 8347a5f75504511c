"""The persistent x3 act's epilogue and addressing (csrc/qmlp.hip qact3p_kernel) at the smallest
launch that selects it.

The kernel's ReLU, dropout keep test, hi / lo split, H1^T store offsets, weight fragment addresses and
table row offsets are written for few vector instructions; per element they are
the 64-row kernel's products in the same order, so Q and the epsilon-greedy actions must be that
kernel's bit for bit. 4 tiles per CU plus 2 rows: the launcher's threshold, every workgroup's first
and steady-state tiles, and a ragged last tile of one row pair. Hash dropout (mode 1, the bench's),
with and without the act workspace; two tiles carry a row off the table path, so the 64-row body
runs them from the workspace's list or from its own re-check."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def act_case():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from evacx.env import DeviceLayout, VecEnv
    from evacx.layout import build_tables, synthetic
    from evacx.qnet import DROPOUT_P, Learner
    R, E0 = 16, 1024
    lay = DeviceLayout(build_tables(synthetic(128, 128, R)), 2276)
    env = VecEnv(lay, E0)
    env.seed([500 + i for i in range(E0)])
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(12)
    for _ in range(5):
        env.step(torch.randint(0, 5, (E0 * R,), device="cuda", dtype=torch.int32, generator=g), auto_reset=True)
    torch.cuda.synchronize()
    lc = lay.c
    t_max = int(lc.t_max)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * ncu * 128 + 2
    rows0 = env.obs.view(-1, 8)
    obs = rows0.repeat((n + rows0.shape[0] - 1) // rows0.shape[0], 1)[:n].contiguous()
    obs[:, 6] = t_max
    # a row below the table's fire step in tile 3 and in the second-to-last full tile: both off the table path
    obs[3 * 128 + 77, 6] = t_max - 1
    obs[(4 * ncu - 2) * 128 + 5, 6] = t_max - 1
    lr = Learner(kind="mlp", precision="f32", seed=23)
    fast = lr.fast
    fast.attach_static(lc, int(lc.L), int(lc.W), t_max, x_range=(max(lc.rx_lo, 0), min(lc.rx_hi, lc.L + 1)))
    base = dict(drop=(31, 9, DROPOUT_P), epsilon=0.1, act_seed=6, act_offset=33)

    def run(kernel64, ws):
        q = torch.full((n, 5), float("nan"), device="cuda")
        a = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        args = dict(q=q, actions=a, kernel64=kernel64, ws=ws, **base)
        plan = fast.act_plan(lc, obs.view(-1), n, **args)
        fast.act(lc, obs.view(-1), n, **args)
        torch.cuda.synchronize()
        return plan, q, a

    _, q64, a64 = run(True, None)  # the reference, computed once
    assert torch.isfinite(q64).all() and (a64 >= 0).all()
    return dict(n=n, ncu=ncu, run=run, q64=q64, a64=a64, keep=(lay, env, lr))


@pytest.mark.parametrize("workspace", [False, True])
def test_persistent_act_at_threshold_matches_64_row_kernel(act_case, workspace):
    from evacx._lib import FWD
    from evacx.qmlp import act_ws_ints
    n, ncu = act_case["n"], act_case["ncu"]
    ws = torch.zeros(act_ws_ints(n), dtype=torch.int32, device="cuda") if workspace else None
    plan, q, a = act_case["run"](False, ws)
    assert plan.route == FWD["ACT_PERSISTENT"], plan.route
    assert plan.drop_mode == 1 and 0 < plan.act_grid <= ncu and plan.rest_listed == int(workspace)
    assert torch.equal(q, act_case["q64"])
    assert torch.equal(a, act_case["a64"])
    if workspace:
        assert ws[:2].tolist() == [0, 0]  # the count and the done counter, reset for the next act


def test_one_tile_fewer_takes_the_64_row_kernel(act_case):
    """The launch above is the smallest: with one tile fewer per chip the plan is the 64-row kernel."""
    from evacx._lib import FWD
    lay, env, lr = act_case["keep"]
    n = act_case["n"] - 2 - 128
    obs = env.obs.view(-1, 8)
    obs = obs.repeat((n + obs.shape[0] - 1) // obs.shape[0], 1)[:n].contiguous()
    q = torch.empty(n, 5, device="cuda")
    plan = lr.fast.act_plan(lay.c, obs.view(-1), n, drop=(31, 9, 0.2), q=q)
    assert plan.route == FWD["ACT_64"], plan.route


# ---------------------------------------------------------------- the saved H1 planes, bit for bit
# The online forward that saves its H1 planes for the backward (evx_qmlp_forward with out.h1, H2 and Q)
# at B = 64, 66 and 130 rows: one 64-row tile, a ragged pair, a ragged third tile. At these sizes the
# launcher's route is qfc1_kernel + qfc23_kernel, so the epilogue under test is fc1_slab_m -- the one the
# 64-row act kernels (act3h_tile, with or without SAVE) share; the act-kernel SAVE route itself starts
# at 32 768 rows (fwd_plan) and is covered by tests/test_target_table_gpu.py.
#
# fc1's weights are set so that every pre-activation is exact in float32 and in hi + lo: only the
# columns of the window channels whose inputs are all 0 or 1 are non-zero, weights and biases are k / 256 with |k| <= 64 (the scale of a trained
# layer), so z is a sum of at most 485 such terms (|z| < 128, 8 fractional bits: 15 significant bits) in any order.
# relu(z) is then hi + lo of the same launch without dropout, exactly, and the planes with dropout must
# be split2(relu(z) * keep * scale) bit for bit, keep from oracle.dropout_keep.
T16 = int(0.2 * 65536.0)  # thresh16 of p = 0.2


def _uniform_is(seed, stream, t, rows):
    """[rows][512] bool: the element's 16-bit uniform equals t (kept at threshold t, dropped at t + 1)."""
    from oracle import oracle as orc
    return (orc.dropout_keep(seed, stream, t / 65536.0, rows) != 0) & (orc.dropout_keep(seed, stream, (t + 1) / 65536.0, rows) == 0)


def _boundary_seed(stream, rows):
    """The first seed whose batch holds a uniform equal to thresh16 and one equal to thresh16 - 1 (CPU only)."""
    for seed in range(1, 200):
        if _uniform_is(seed, stream, T16, rows).any() and _uniform_is(seed, stream, T16 - 1, rows).any():
            return seed
    raise AssertionError("no seed with both boundary uniforms")


def _split2(v):
    hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


@pytest.fixture(scope="module")
def save_case():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from evacx.env import DeviceLayout, VecEnv
    from evacx.layout import build_tables, synthetic
    from evacx.qmlp import HID, K1
    from evacx.qnet import Learner
    R, E = 2, 65
    lay = DeviceLayout(build_tables(synthetic(48, 48, R)), 600)
    env = VecEnv(lay, E)
    env.seed([40 + i for i in range(E)])
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(2)
    for _ in range(5):
        env.step(torch.randint(0, 5, (E * R,), device="cuda", dtype=torch.int32, generator=g))
    torch.cuda.synchronize()
    lr = Learner(kind="mlp", precision="f32", seed=19)
    assert lr.fast.x3
    gw = torch.Generator().manual_seed(4)
    X = env.expand_obs(torch.float32).reshape(E * R, K1)
    # the window channels whose every value is 0 or 1 (channel 0 is identically 0, 5 the centre one-hot)
    Xc = X.view(-1, 121, 6)
    binary = [c for c in range(1, 5) if bool(((Xc[:, :, c] == 0) | (Xc[:, :, c] == 1)).all()) and Xc[:, :, c].sum().item() > 0]
    assert binary, "no 0 / 1 input channel to build exact pre-activations from"
    w1 = torch.zeros(HID, K1)
    for c in binary:
        w1.view(HID, 121, 6)[:, :, c] = torch.randint(-64, 65, (HID, 121), generator=gw).float() / 256
    lr.online["fc1.weight"].copy_(w1.cuda())  # (views of the flat parameter buffer)
    lr.online["fc1.bias"].copy_((torch.randint(-64, 65, (HID,), generator=gw).float() / 256).cuda())
    lr.fast.repack()
    return dict(lay=lay, env=env, lr=lr, X=X)


@pytest.mark.parametrize("B", [64, 66, 130])
def test_saved_h1_planes_are_split2_of_relu_keep_scale(save_case, B):
    import torch.nn.functional as F
    from evacx.qmlp import HID, K1X
    from oracle import oracle as orc
    lay, env, lr, X = (save_case[k] for k in ("lay", "env", "lr", "X"))
    fast, dev, stream = lr.fast, "cuda", 3
    seed = _boundary_seed(stream, B)

    def run(p):
        h1 = torch.full((2 * B * HID,), 0x7fc0, dtype=torch.int16, device=dev)
        x = torch.empty(B * K1X, dtype=torch.int16, device=dev)
        h2 = torch.empty(B, 256, device=dev)
        q = torch.full((B, 5), float("nan"), device=dev)
        fast.forward(lay.c, env.obs, B, h1, drop=(seed, stream, p), x=x, h2=h2, q=q)
        torch.cuda.synchronize()
        pl = h1.view(torch.bfloat16).view(2, B, HID)
        return pl[0], pl[1], q

    hi0, lo0, q0 = run(0.0)
    r = hi0.float() + lo0.float()  # relu(z), exact: the planes of r are the planes read
    eh, el = _split2(r)
    assert torch.equal(eh.view(torch.int16), hi0.view(torch.int16)) and torch.equal(el.view(torch.int16), lo0.view(torch.int16))
    ref1 = torch.relu(torch.nn.functional.linear(X[:B], lr.online.state_dict()["fc1.weight"], lr.online.state_dict()["fc1.bias"]))
    assert torch.equal(r, ref1)  # exact by construction (torch's f32 sum of the same dyadic terms)
    assert (r > 0).float().mean().item() > 0.1 and (r == 0).float().mean().item() > 0.1

    hi1, lo1, q1 = run(0.2)
    keep_np = orc.dropout_keep(seed, stream, 0.2, B) != 0
    at_t, below_t = _uniform_is(seed, stream, T16, B), _uniform_is(seed, stream, T16 - 1, B)
    assert at_t.any() and below_t.any()  # both sides of the keep test's boundary are in the batch
    assert keep_np[at_t].all() and not keep_np[below_t].any()
    keep = torch.from_numpy(keep_np).to(dev)
    scale = torch.tensor(1.0, dtype=torch.float32) / (1.0 - torch.tensor(0.2, dtype=torch.float32))
    v = torch.where(keep, r * scale.item(), torch.zeros_like(r))
    eh, el = _split2(v)
    assert torch.equal(eh.view(torch.int16), hi1.view(torch.int16))
    assert torch.equal(el.view(torch.int16), lo1.view(torch.int16))
    # Q against torch fp32 on the expanded observations, the existing x3 bars (tests/test_qmlp_x3_gpu.py)
    sd = lr.online.state_dict()
    for q, mask in ((q0, None), (q1, keep.to(torch.uint8))):
        h = ref1 if mask is None else ref1 * mask.float() / 0.8  # agents/dqn_agent.py:40-61's fc stack
        refq = F.linear(F.relu(F.linear(h, sd["fc2.weight"], sd["fc2.bias"])), sd["fc3.weight"], sd["fc3.bias"])
        torch.testing.assert_close(q, refq, rtol=2e-4, atol=2e-5)
