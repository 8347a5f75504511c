"""The grouped learn chain (evacx.qgroup.GroupedLearner: evx_qmlp_forward2_g -> evx_td_loss_zero_g ->
evx_qmlp_backward_ss_g -> evx_qmlp_adam_pack3_g, csrc/qmlp.hip and csrc/qnet.hip) against torch
float64 per net, at the net counts and batch sizes where its launch shape changes.

The chain takes its launch shape from the same B-dependent rules as the single net (qbwd3's rows per
block, the split counts of dW1 and dW2, dZ1's tiles per workgroup) and, on top, per-net pointer
strides (fwd_net, bwd_net, gsA / gsB / gsC / gsP of the split-K GEMMs, the TD partials' [net][block]
index). A wrong stride does not crash: it reads the neighbour's rows or partials and gives plausible
numbers. So every net of a case has its own seed (online and target), its own rows, and is compared
with its own float64 reference (tests/learn_util.py: that net's parameters, moments, keep masks and
the device's own gates); the per-net losses must be pairwise distinct.

Each case names the plan fields it is there for; evx_qmlp_group_plan (the launchers' own decision
function, pinned in test_qgroup_plan_cpu.py) must report them, so a re-tuned threshold fails the case
instead of leaving it testing another route. Bars: the x3 path's (learn_util.check_*), not re-tuned."""
import ctypes as C

import pytest
import torch

import learn_util as lu

pytestmark = pytest.mark.gpu

ROWS = 4096  # one env serves the module; grouped batches draw from it with replacement


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _grouped(G, seed):
    """A GroupedLearner whose nets differ (seed + g) and whose target nets differ from the online
    ones from the first step on (seed + 1000 + g, operands repacked)."""
    from evacx.qgroup import GroupedLearner
    grp = GroupedLearner(G, seed=seed, lr=1e-3)
    for g in range(G):
        grp.target[g].init_like_torch(seed + 1000 + g)
    grp.fast_t.repack()
    return grp


def _assert_plan(G, B, want):
    from evacx.qgroup import group_plan
    p = group_plan(B, G)
    got = {k: getattr(p, k) for k in want}
    assert got == want, f"G={G} B={B}: this case no longer runs the route it names: {got}, named {want}"


# (G, B, dropout p, the plan fields the case is there for)
SWEEP = [
    (2, 2, 0.2, dict(fc1_rows=64, qbwd3_rows=32, dw1_gz=1, dw2_gz=1, td_blocks=1)),  # one row pair, one block
    (3, 258, 0.2, dict(td_blocks=2, dw1_gz=5, dw2_gz=5)),  # a second TD block of two rows per net; 5 splits, the last short
    (3, 258, 0.0, dict(td_blocks=2)),                      # dropout off
    (16, 1408, 0.2, dict(fc1_rows=64)),                    # last B on the 64-row fc1 at G = 16
    (16, 1410, 0.2, dict(fc1_rows=128, td_blocks=6)),      # first B on the 128-row fc1: its twelfth tile holds two rows
    (32, 642, 0.2, dict(fc1_rows=128, dw1_gz=6)),          # the 128-row fc1 at 32 nets, ragged sixth tile
    (2, 2050, 0.2, dict(qbwd3_rows=16, dw1_gz=7)),         # the 16-row band; a tail block of two rows
    (2, 4098, 0.2, dict(qbwd3_rows=16, dw1_kper=576, dw1_gz=8, dw2_kper=320, dw2_gz=13)),  # dW1's split rule switches
    (2, 8194, 0.2, dict(qbwd3_rows=64, qdz1_tiles=2, dw2_gz=26)),  # 64-row band; a short last dZ1 workgroup
    (2, 16386, 0.2, dict(qbwd3_rows=128, qdz1_tiles=4, fc1_rows=128, td_blocks=65)),  # 128-row band, two-row tail
    (64, 2, 0.2, dict(fc1_rows=64, td_blocks=1)),          # the most nets GroupedLearner takes
]


@pytest.mark.parametrize("G,B,drop_p,plan", SWEEP, ids=[f"{g}x{b}{'' if p else '-nodrop'}" for g, b, p, _ in SWEEP])
def test_grouped_learn_step_matches_float64_per_net(G, B, drop_p, plan):
    """Two grouped learn steps, sync_target() between them (the target operands repacked), each net of
    each step against DQNAgent.learn in float64 from that net's state before the step: the bars of
    test_learn_batch_sweep_gpu.py::test_x3_learn_step_matches_float64_at_B (check_flips,
    check_loss_and_grads, check_adam), per net; the nets' losses pairwise distinct."""
    _need_gpu()
    _assert_plan(G, B, plan)
    lay, env = lu.small_env(ROWS)
    grp = _grouped(G, 300 + G)
    grp.drop_p = drop_p
    gen = torch.Generator().manual_seed(7000 + 31 * G + B)
    for it in range(2):
        gb = lu.grouped_batch(env, G, B, gen)
        pairs = lu.grouped_step_and_references(grp, lay, env, gb)
        for g, (dev, ref) in enumerate(pairs):
            what = f"G={G} B={B} p={drop_p} step {it} net {g}"
            lu.check_flips(ref, what)
            lu.check_loss_and_grads(dev, ref, what)
            lu.check_adam(dev, ref, what)
        losses = [dev.loss for dev, _ in pairs]
        assert len(set(losses)) == G, f"G={G} B={B} step {it}: two nets with one loss: {losses}"
        if it == 0:
            grp.sync_target()
            assert torch.equal(grp.tflat, grp.flat)


def _canary(shape, dtype, live):
    """A buffer of `shape` filled with canaries (f32: NaN, int16: the bf16 NaN 0x7fc0); elements from
    `live` on (flat) are expected to keep them. Returns (buffer, canary view as integers, its copy)."""
    if dtype == torch.float32:
        t = torch.full(shape, float("nan"), device="cuda")
        bits = t.view(-1).view(torch.int32)
    else:
        t = torch.full(shape, 0x7fc0, dtype=torch.int16, device="cuda")
        bits = t.view(-1)
    tail = bits[live:]
    return t, tail, tail.clone()


@pytest.mark.parametrize("G,B", [(3, 190), (2, 2050)])
def test_grouped_learn_keeps_to_its_rows(G, B):
    """The _g entry points called directly on caller buffers [G + 1][one net's size]: X, both nets'
    H1 planes, H2, Q, Qt, dQ, dZ1, dZ2, the split-K partials, the TD partials and the gradients, all
    pre-filled with canaries (NaN; bf16: 0x7fc0). Everything behind net G - 1 keeps its bits (the
    gradient clear of evx_td_loss_zero_g stops at G nets too), and every net's loss and raw gradients
    are finite and within the bars of the sweep -- a slice that reached past its net's rows or
    partials would carry a NaN."""
    _need_gpu()
    from evacx._lib import evx_qmlp_grads, lib
    from evacx.env import _stream
    from evacx.qmlp import HID, HID2, K1X, NACT, MLPFast
    from evacx.qnet import FlatParams
    lay, env = lu.small_env(ROWS)
    grp = _grouped(G, 500 + G)
    L = lib()
    npar, nss = grp.npar, grp.nss
    pf, ntd = int(L.evx_qmlp_backward_part_floats(B)), int(L.evx_td_loss_ws_floats(B, 1))
    assert int(L.evx_td_loss_ws_floats(B, G)) == G * ntd
    i16, f32 = torch.int16, torch.float32
    sizes = {"x": (B * K1X, i16), "h1": (2 * B * HID, i16), "h1t": (2 * B * HID, i16), "h2": (B * HID2, f32),
             "q": (B * NACT, f32), "qt": (B * NACT, f32), "dq": (B * NACT, f32), "dz1": (2 * B * HID, i16),
             "dz2": (2 * B * HID2, i16), "part": (pf, f32), "td_ws": (ntd, f32), "grads": (npar, f32)}
    bufs = {k: _canary((G + 1, n), dt, G * n) for k, (n, dt) in sizes.items()}
    t = {k: v[0] for k, v in bufs.items()}
    loss = torch.full((G + 1,), float("nan"), device="cuda")
    ss = torch.full((G + 1, nss), float("nan"), device="cuda")
    gb = lu.grouped_batch(env, G, B, torch.Generator().manual_seed(8000 + B))
    seed, stream, p = 11, 6, 0.2
    d_on, d_tg = MLPFast._drop((seed, stream, p)), MLPFast._drop((seed, stream + 1, p))
    o_on, o_tg = MLPFast._out(t["h1"], t["x"], t["h2"], t["q"]), MLPFast._out(t["h1t"], None, None, t["qt"])
    rc = L.evx_qmlp_forward2_g(C.byref(lay.c), B, G, gb.s.data_ptr(), C.byref(grp.fast.c), C.byref(d_on), C.byref(o_on),
                               gb.s2.data_ptr(), C.byref(grp.fast_t.c), C.byref(d_tg), C.byref(o_tg), _stream())
    assert rc == 0, L.evx_last_error()
    rc = L.evx_td_loss_zero_g(t["q"].data_ptr(), t["qt"].data_ptr(), NACT, gb.a.data_ptr(), gb.r.data_ptr(),
                              gb.d.data_ptr(), grp.gamma, B, G, None, t["dq"].data_ptr(), loss.data_ptr(), None,
                              t["grads"].data_ptr(), G * npar, t["td_ws"].data_ptr(), G * ntd, _stream())
    assert rc == 0, L.evx_last_error()
    g0 = FlatParams(grp.shapes, grp.device, data=t["grads"][0])
    gr = evx_qmlp_grads(w1=g0["fc1.weight"].data_ptr(), b1=g0["fc1.bias"].data_ptr(), w2=g0["fc2.weight"].data_ptr(),
                        b2=g0["fc2.bias"].data_ptr(), w3=g0["fc3.weight"].data_ptr(), b3=g0["fc3.bias"].data_ptr(),
                        part=t["part"].data_ptr())
    rc = L.evx_qmlp_backward_ss_g(C.byref(grp.fast.c), B, G, t["dq"].data_ptr(), t["x"].data_ptr(), t["h1"].data_ptr(),
                                  t["h2"].data_ptr(), p, t["dz2"].data_ptr(), t["dz1"].data_ptr(), C.byref(gr),
                                  ss.data_ptr(), _stream())
    assert rc == 0, L.evx_last_error()
    torch.cuda.synchronize()
    for k, (_, tail, want) in bufs.items():
        assert torch.equal(tail, want), f"G={G} B={B}: {k} written behind net {G - 1}"
    assert torch.isnan(loss[G]) and bool(torch.isnan(ss[G]).all()), "loss / norm partials written behind the last net"
    m1, m2 = lu.grouped_keep_masks(seed, stream, p, G, B, loss.device)
    losses = []
    for g in range(G):
        g1, g2 = lu.net_gates(t["h1"].view(-1), t["h2"].view(-1), g, B)
        ref = lu.float64_reference(env, grp.online[g].state_dict(), grp.target[g].state_dict(),
                                   lu.net_batch(gb, g, m1, m2), g1, g2)
        dev = lu.SimpleNamespace(loss=loss[g].item(), norm=float(ss[g].double().sum().sqrt()),
                                 grads=FlatParams(grp.shapes, grp.device, data=t["grads"][g]).state_dict(), td_abs=None)
        what = f"G={G} B={B} canaries net {g}"
        lu.check_flips(ref, what)
        lu.check_loss_and_grads(dev, ref, what)
        losses.append(dev.loss)
    assert len(set(losses)) == G, losses


@pytest.mark.parametrize("G,B", [(16, 1410), (2, 8194)])
def test_grouped_learn_is_deterministic(G, B):
    """Two GroupedLearners stepped twice from the same state on the same batches: bit-equal losses,
    norms, gradients, parameters and Adam moments. Every sum of the chain runs in a fixed order (the
    TD partials in block order, the split-K slices in z order per net)."""
    _need_gpu()
    lay, env = lu.small_env(ROWS)
    gen = torch.Generator().manual_seed(9000 + B)
    batches = [lu.grouped_batch(env, G, B, gen) for _ in range(2)]
    runs = []
    for _ in range(2):
        grp = _grouped(G, 700 + G)
        out = []
        for gb in batches:
            loss = grp.learn_obs(lay.c, gb.s, gb.a, gb.r, gb.d, gb.s2, B)
            torch.cuda.synchronize()
            out += [loss.clone(), grp.norm.clone(), grp.gflat.clone(), grp.flat.clone(), grp.m.clone(), grp.v.clone()]
        runs.append(out)
    names = [f"step {s} {n}" for s in range(2) for n in ("loss", "norm", "gflat", "flat", "m", "v")]
    for name, x, y in zip(names, *runs):
        assert torch.isfinite(x).all(), name
        assert torch.equal(x, y), f"G={G} B={B}: {name} differs between two runs from the same state"
