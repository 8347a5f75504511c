"""The grouped learn chain's launch plan (evx_qmlp_group_plan: the function qmlp_backward and
launch_tail take their decisions from, fc1's rows by the forward plan's rule) pinned at every band edge, and the
argument refusals of the grouped act and of the mixer -- all on a host without a GPU: none of these
calls launches or touches a device.

The expected figures restate the rules of csrc/qmlp.hip by hand:
* fc1: 128-row tiles from ceil(B / 128) x 2 problems x nets >= 384, else 64-row;
* qbwd3_rows: 32 up to 2048, 16 below 8192, 64 below 16384, 128 from there;
* K splits (ksplit_kper): S = max(8, min(slots / tiles, B / minrows) rounded down to 8s), kper =
  ceil(B / S) rounded up to 64, gz = ceil(B / kper); dW1 (x3): 20 tiles, 512 slots, minrows 256 up to
  B = 4096 and 1024 above; dW2: 8 tiles, 256 slots, minrows 256;
* qdz1 tiles per workgroup: B / 4096 clamped to 1..8;
* TD blocks per net: ceil(B / 256).
tests/test_qgroup_sweep_gpu.py asserts through the same query that each of its cases runs the route
it names, so a re-tuned threshold fails here (the pin) and there (the case's route)."""
import ctypes

import pytest

FAKE = 0x1000  # a non-null address that is never dereferenced


def _plan(B, nets):
    from evacx.qgroup import group_plan
    p = group_plan(B, nets)
    return (p.fc1_rows, p.qbwd3_rows, p.dw1_kper, p.dw1_gz, p.dw2_kper, p.dw2_gz, p.qdz1_tiles, p.td_blocks)


# (nets, B): fc1 rows, qbwd3 rows, dW1 kper, dW1 gz, dW2 kper, dW2 gz, qdz1 tiles, TD blocks
PINS = {
    # the cases of the GPU sweep
    (2, 2): (64, 32, 64, 1, 64, 1, 1, 1),
    (3, 258): (64, 32, 64, 5, 64, 5, 1, 2),            # 5 splits, the last of 2 rows; a second TD block
    (16, 1408): (64, 32, 192, 8, 192, 8, 1, 6),        # 11 tiles x 32 = 352 < 384
    (16, 1410): (128, 32, 192, 8, 192, 8, 1, 6),       # 12 x 32 = 384
    (32, 642): (128, 32, 128, 6, 128, 6, 1, 3),        # 6 x 64 = 384
    (2, 2050): (64, 16, 320, 7, 320, 7, 1, 9),
    (2, 4098): (64, 16, 576, 8, 320, 13, 1, 17),       # dW1 on one split per 1024 rows, dW2 per 256
    (2, 8194): (64, 64, 1088, 8, 320, 26, 2, 33),
    (2, 16386): (128, 128, 1088, 16, 576, 29, 4, 65),  # 129 x 4 = 516 tiles
    (64, 2): (64, 32, 64, 1, 64, 1, 1, 1),
    # the other side of each edge
    (32, 640): (64, 32, 128, 5, 128, 5, 1, 3),         # 5 x 64 = 320
    (4, 6016): (64, 16, 768, 8, 384, 16, 1, 24),       # 47 x 8 = 376
    (4, 6018): (128, 16, 768, 8, 384, 16, 1, 24),      # 48 x 8 = 384
    (2, 256): (64, 32, 64, 4, 64, 4, 1, 1),
    (2, 2048): (64, 32, 256, 8, 256, 8, 1, 8),
    (2, 4096): (64, 16, 256, 16, 256, 16, 1, 16),      # the last B on dW1's 256-row rule
    (2, 8190): (64, 16, 1024, 8, 384, 22, 1, 32),
    (2, 8192): (64, 64, 1024, 8, 256, 32, 2, 32),
    (2, 16382): (128, 64, 2048, 8, 512, 32, 3, 64),
    (2, 16384): (128, 128, 1024, 16, 512, 32, 4, 64),
    (2, 32768): (128, 128, 1408, 24, 1024, 32, 8, 128),
    (2, 65536): (128, 128, 2752, 24, 2048, 32, 8, 256),
    # one net: the single-net backward's figures
    (1, 4096): (64, 16, 256, 16, 256, 16, 1, 16),
    (1, 32768): (128, 128, 1408, 24, 1024, 32, 8, 128),
}


@pytest.mark.parametrize("nets,B", sorted(PINS), ids=[f"{g}x{b}" for g, b in sorted(PINS)])
def test_group_plan_at_the_band_edges(nets, B):
    assert _plan(B, nets) == PINS[(nets, B)]


def _restated(B, nets):
    def kper(tiles, slots, minrows):
        S = max(8, min(slots // tiles // 8 * 8, B // minrows // 8 * 8))
        return -(-(-(-B // S)) // 64) * 64
    k1, k2 = kper(20, 512, 256 if B <= 4096 else 1024), kper(8, 256, 256)
    return (128 if -(-B // 128) * 2 * nets >= 384 else 64,
            128 if B >= 16384 else 64 if B >= 8192 else 16 if B > 2048 else 32,
            k1, -(-B // k1), k2, -(-B // k2), min(max(B // 4096, 1), 8), -(-B // 256))


def test_group_plan_follows_the_restated_rules_everywhere():
    """Every B up to 2^15 + 2 at 1, 2, 16, 32 and 64 nets, and the pins themselves, against the
    module docstring's rules written out in Python."""
    for (nets, B), want in PINS.items():
        assert _restated(B, nets) == want, (nets, B)
    for nets in (1, 2, 16, 32, 64):
        for B in list(range(1, 2600)) + list(range(3900, 4300)) + list(range(8000, 8400)) + \
                list(range(16200, 16500)) + [32766, 32768, 32770]:
            assert _plan(B, nets) == _restated(B, nets), (nets, B)


def test_group_plan_refuses_bad_arguments():
    from evacx import _lib
    L = _lib.lib()
    p = _lib.evx_qmlp_plan(*[7] * 8)
    for B, nets, text in ((2, 0, b"nets must be 1..1024"), (2, -1, b"nets must be 1..1024"),
                          (2, 1025, b"nets must be 1..1024"), (0, 2, b"B must be > 0"), (-2, 2, b"B must be > 0")):
        assert L.evx_qmlp_group_plan(B, nets, ctypes.byref(p)) == -22
        assert text in L.evx_qmlp_last_error(), (B, nets, L.evx_qmlp_last_error())
        assert _plan_tuple(p) == (0,) * 8  # a refused query leaves no stale figures
    assert L.evx_qmlp_group_plan(2, 2, None) == -22 and b"NULL plan" in L.evx_qmlp_last_error()
    with pytest.raises(_lib.EvacxError, match="nets must be 1..1024"):
        _plan(2, 0)


def _plan_tuple(p):
    return tuple(getattr(p, n) for n, _ in p._fields_)


def test_grouped_act_refuses_odd_rows_permutation_and_table():
    """evx_qmlp_act_g's checks come before anything is read: fake pointers, no device."""
    from evacx import _lib
    L = _lib.lib()
    lay = _lib.evx_layout()
    drop = _lib.evx_qmlp_dropout(seed=1, stream=2, p=0.2)

    def act(n, nets, par, out):
        return L.evx_qmlp_act_g(ctypes.byref(lay), FAKE, n, nets, ctypes.byref(par), ctypes.byref(drop),
                                ctypes.byref(out), None)
    x3 = _lib.evx_qmlp_params(x3=1)
    q = _lib.evx_qmlp_fwd_out(q=FAKE)
    for n, nets, par, out, text in (
            (63, 16, x3, q, b"qmlp_act_g: rows per net must be even (dropout row pairs)"),
            (1, 32, x3, q, b"qmlp_act_g: rows per net must be even (dropout row pairs)"),
            (62, 16, x3, _lib.evx_qmlp_fwd_out(q=FAKE, perm=FAKE), b"qmlp_act_g: no act permutation with grouped nets"),
            (62, 16, _lib.evx_qmlp_params(x3=1, stat=FAKE), q, b"qmlp_act_g: the act table path is single-net"),
            (62, 16, x3, _lib.evx_qmlp_fwd_out(), b"qmlp_act_g: needs q or actions"),
            (62, 0, x3, q, b"grouped qmlp: nets must be 1..1024"),
            (62, 16, _lib.evx_qmlp_params(x3=0), q, b"grouped qmlp: x3 parameters required")):
        assert act(n, nets, par, out) == -22, text
        assert text in L.evx_qmlp_last_error(), (text, L.evx_qmlp_last_error())
    assert act(0, 16, x3, q) == 0  # no rows: nothing to do


def test_grouped_learner_refuses_net_counts():
    """GroupedLearner takes 1..64 nets (refused before any device is reached)."""
    from evacx.qgroup import GroupedLearner
    for nets in (0, 65):
        with pytest.raises(ValueError, match="1..64 nets"):
            GroupedLearner(nets, device="cpu")


@pytest.mark.parametrize("n,A,text", [(0, 5, b"qmix_loss: 1..16 agents"), (17, 5, b"qmix_loss: 1..16 agents"),
                                      (-1, 5, b"qmix_loss: 1..16 agents"), (16, 0, b"qmix_loss: 1..64 actions"),
                                      (16, 65, b"qmix_loss: 1..64 actions"), (1, 1, b"qmix_loss: NULL argument")])
def test_qmix_loss_refuses_agent_and_action_counts(n, A, text):
    from evacx import _lib
    L = _lib.lib()
    ptr = [FAKE] * 11 if text != b"qmix_loss: NULL argument" else [FAKE] * 10 + [None]
    Q, Qt, act, rew, done, mix, mix_t, dQ, grad, loss, part = ptr
    assert L.evx_qmix_loss(Q, Qt, A, act, rew, done, 0.99, 4, n, mix, mix_t, dQ, grad, loss, part, None, 0, None) == -22
    assert text in L.evx_qmix_last_error(), L.evx_qmix_last_error()


def test_qmix_loss_without_rows_is_a_no_op():
    """B <= 0 returns 0 before any other check or launch (the GPU test checks nothing was written)."""
    from evacx import _lib
    L = _lib.lib()
    for B in (0, -3):
        assert L.evx_qmix_loss(*[None] * 2, 5, *[None] * 3, 0.99, B, 2, *[None] * 7, 0, None) == 0
    assert int(L.evx_qmix_part_floats(0, 2)) == 0 and int(L.evx_qmix_part_floats(257, 16)) == 2 * (16 * 32 + 66)
