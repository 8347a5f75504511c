"""The fused x3 learn step (evx_qmlp_forward2 -> evx_qmlp_td_backward -> evx_qmlp_adam_pack3,
csrc/qmlp.hip) against torch float64 in every batch-size band of its launch shape and at ragged
batches, where the kernels' tail code runs.

The launch shape depends on the batch size B alone: qbwd3_kernel's rows per block (qbwd3_rows:
32 up to 2048, 16 below 8192, 64 below 16384, 128 from there), dW1's split rule (dw1_kper: one split
per 256 rows up to 4096, per 1024 above), the split counts (ksplit_kper: gz = ceil(B / kper) may be
no multiple of 8, and the last split short), dZ1's tiles per workgroup (qdz1_tiles_per_wg), the
forward pair (two kernels below 8192, qfwd2_kernel with act tables from there, the fused act kernel
from 32768). Ragged B: qbwd3's scalar row loop, qdz1_body's row guards and its last workgroup's tile
count, gemm_tn_body's zero-filled rows past the split's end, qfc1 / qfc23 / qfwd2 / x_expand's last tile.
Helpers and the reference: tests/learn_util.py. Bars: the x3 path's (tests/test_qmlp_x3_gpu.py,
test_bench_scale_gpu.py::test_x3_learn_at_bench_batch), not re-tuned here."""
import pytest
import torch

import learn_util as lu

pytestmark = pytest.mark.gpu

ROWS = 2 * 16400  # one env serves every case: E * R >= 2 B at the largest B


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# (B, act tables, prioritized weights + |TD| out). Weights on about every second row, arranged so that
# a.w != NULL and a.w == NULL each meet whole blocks (2048 / 16384 and 4096) and ragged tails, in
# every band of qbwd3_rows.
SWEEP = [
    (1, False, False),      # 32-row band: one row in one block
    (2, False, True),
    (31, False, False),     # a tail row loop, one kper chunk that is not full
    (33, False, True),      # a second block of one row
    (2048, False, True),    # last B of the 32-row band
    (2049, False, False),   # first B of the 16-row band; a one-row tail block on the scalar loop
    (4096, False, False),   # cfg2's batch: whole 16-row blocks, 16 dW1 splits
    (4097, False, True),    # the dW1 split rule switches; ragged in every kernel
    (8191, False, False),   # last B of the 16-row band and of the two-kernel forward
    (8200, False, True),    # 64-row band, ragged
    (8200, True, False),    # ... qfwd2_kernel's last 64-row tile and x_expand_kernel ragged
    (16383, False, False),  # the edge where 128-row blocks begin
    (16384, False, True),
    (16400, False, False),  # 128-row band with a 16-row tail chunk
    (16400, True, True),
]


def _learner(seed):
    from evacx.qnet import Learner
    return Learner(kind="mlp", precision="f32", seed=seed, lr=1e-3)


@pytest.mark.parametrize("B,table,weights", SWEEP,
                         ids=[f"{b}{'t' if t else ''}-{'w' if w else 'u'}" for b, t, w in SWEEP])
def test_x3_learn_step_matches_float64_at_B(B, table, weights):
    """Two learn steps, each from identical parameters and Adam moments on both sides (the
    reference restarts from the device's state), against DQNAgent.learn in torch float64 on the
    expanded observations through the device's own ReLU / dropout branches:
    loss rtol 2e-4 (+1e-5) against the gated and the plain reference; norm rtol 2e-4 (gated), 1e-3
    (plain); every gradient rtol 2e-3, atol 1e-5 max |grad| + 1e-9; |TD| rtol 2e-4, atol 2e-5; Adam:
    at most 1e-3 of a tensor's elements beyond 1e-5, none beyond 2e-3; the branches that differ from
    plain torch's within 1e-4 of the layer's max |z| and at most max(2, 1e-5 x activations)."""
    _need_gpu()
    lay, env = lu.small_env(ROWS)
    lr = _learner(41)
    if table:
        lu.attach_tables(lr, lay)
    # which forward pair ran: qfwd2_kernel keeps the target's H1 in LDS, qfc1 + qfc23 write its planes
    from evacx._lib import FWD
    from evacx.qmlp import HID
    h1t = lr.net.ws.get("fh1t", (B * 2 * HID,), torch.int16, lr.device).fill_(0x7fc0)
    gen = torch.Generator().manual_seed(1000 + B)
    for it in range(2):
        bt = lu.make_batch(env, lay, B, gen, table=table, weights=weights, td_abs=weights)
        # the forward pair this case names (the module docstring's bands), asked of the launcher's own plan
        plan = lr.learn_plan(lay.c, bt.s_obs, bt.s2_obs, B, mask_online=bt.m1, mask_target=bt.m2)
        assert (plan.route, plan.x_expand) == ((FWD["PAIRED"], 1) if table and B >= 8192 else (FWD["FC"], 0)), \
            f"B={B} table={table}: this case no longer runs the forward pair it names"
        assert plan.fc1_rows == (0 if table and B >= 8192 else 64)  # every B here is below 384 128-row tiles
        assert plan.fc23_rows == (0 if table and B >= 8192 else 32 if -(-B // 64) * 2 < 256 else 64)
        dev, ref = lu.learn_step_and_reference(lr, lay, env, bt)
        what = f"B={B} table={table} weights={weights} step {it}"
        lu.check_flips(ref, what)
        lu.check_loss_and_grads(dev, ref, what)
        lu.check_adam(dev, ref, what)
    paired = not bool((h1t != 0x7fc0).any())
    assert paired == (table and B >= 8192), f"B={B} table={table}: this case no longer runs the forward pair it names"


def _canary(rows_used, rows_all, per_row, dtype):
    """A buffer of rows_all rows whose elements past rows_used rows are canaries: NaN (f32), the
    bf16 NaN pattern 0x7fc0 (int16). Returns (buffer, canary view, its expected bits)."""
    if dtype == torch.float32:
        t = torch.full((rows_all * per_row,), float("nan"), device="cuda")
        bits = t.view(torch.int32)
    else:
        t = torch.full((rows_all * per_row,), 0x7fc0, dtype=torch.int16, device="cuda")
        bits = t
    tail = bits[rows_used * per_row:]
    return t, tail, tail.clone()


@pytest.mark.parametrize("B", [33, 2049, 8200])
def test_learn_step_keeps_to_its_rows(B):
    """forward_pair + td_backward on caller buffers of B + 128 rows (X, both nets' H1 planes, H2, Q, Qt,
    |TD|, dZ1, dZ2): every element past what B rows need (two-plane buffers: past 2 x B x width, the
    lo plane starting at B x width) keeps its canary bits, and the loss and the raw gradients are
    finite and within the bars of test_x3_learn_step_matches_float64_at_B -- a slice that read past
    row B would carry a NaN into dW1 or dW2."""
    _need_gpu()
    from evacx.qmlp import HID, HID2, K1X, NACT, MLPFast
    from evacx.qnet import DROPOUT_P
    lay, env = lu.small_env(ROWS)
    lr = _learner(43)
    bt = lu.make_batch(env, lay, B, torch.Generator().manual_seed(2000 + B), weights=True, td_abs=False)
    n = B + 128
    bufs = {"x": _canary(B, n, K1X, torch.int16), "h1": _canary(2 * B, 2 * n, HID, torch.int16),
            "h1t": _canary(2 * B, 2 * n, HID, torch.int16), "h2": _canary(B, n, HID2, torch.float32),
            "q": _canary(B, n, NACT, torch.float32), "qt": _canary(B, n, NACT, torch.float32),
            "td_abs": _canary(B, n, 1, torch.float32), "dz1": _canary(2 * B, 2 * n, HID, torch.int16),
            "dz2": _canary(2 * B, 2 * n, HID2, torch.int16)}
    t = {k: v[0] for k, v in bufs.items()}
    loss = torch.zeros(1, device="cuda")
    MLPFast.forward_pair(lay.c, B, lr.fast, bt.s_obs, (0, 0, DROPOUT_P, bt.m1, 0),
                         dict(h1=t["h1"], x=t["x"], h2=t["h2"], q=t["q"]), lr.fast_t, bt.s2_obs,
                         (0, 1, DROPOUT_P, bt.m2, 0), dict(h1=t["h1t"], q=t["qt"]))
    lr.fast.td_backward(B, t["q"], t["qt"], bt.a, bt.r, bt.d, lr.gamma, loss, t["x"], t["h1"], t["h2"], DROPOUT_P,
                        t["dz2"], t["dz1"], lr.grads, weights=bt.w, td_abs=t["td_abs"], ss=lr._ss)
    torch.cuda.synchronize()
    for k, (_, tail, want) in bufs.items():
        assert torch.equal(tail, want), f"B={B}: {k} written past its {B} rows"
    from evacx._lib import lib
    norm = float(lr._ss[:int(lib().evx_qmlp_norm_parts())].double().sum().sqrt())
    g1, g2 = lu.device_gates(t["h1"], t["h2"], B)
    bt.td_abs = t["td_abs"][:B]
    ref = lu.float64_reference(env, lr.online.state_dict(), lr.target.state_dict(), bt, g1, g2)
    dev = lu.SimpleNamespace(loss=loss.item(), norm=norm, grads=lr.grads.state_dict(), td_abs=bt.td_abs)
    lu.check_flips(ref, f"B={B}")
    lu.check_loss_and_grads(dev, ref, f"B={B} canaries")


@pytest.mark.parametrize("B", [2049, 4097, 16400])
def test_ragged_learn_is_deterministic(B):
    """Two learners from the same state on the same batch: bit-equal loss, gradients and
    parameters. Every gradient sum runs in a fixed order (reduce2_kernel adds the split-K
    slices in z order); here gz is no multiple of 8 (tn_place's plain order) and the last split short."""
    _need_gpu()
    lay, env = lu.small_env(ROWS)
    bt = lu.make_batch(env, lay, B, torch.Generator().manual_seed(3000 + B), weights=True, td_abs=True)
    runs = []
    for _ in range(2):
        lr = _learner(45)
        bt.td_abs.fill_(float("nan"))
        loss = lr.learn_obs(lay.c, bt.s_obs, bt.a, bt.r, bt.d, bt.s2_obs, B, weights=bt.w, td_abs=bt.td_abs,
                            mask_online=bt.m1, mask_target=bt.m2)
        torch.cuda.synchronize()
        runs.append((loss.clone(), lr.norm.clone(), lr.grads.flat.clone(), lr.online.flat.clone(), bt.td_abs.clone()))
    for name, x, y in zip(("loss", "norm", "grads.flat", "online.flat", "td_abs"), *runs):
        assert torch.isfinite(x).all(), name
        assert torch.equal(x, y), f"B={B}: {name} differs between two runs from the same state"
