"""evx_replay_sample_nstep_agents (csrc/replay.hip: the per-agent / joint draw and the n-step chain in
one launch) against its numpy restatement (tests/marl_opts_util.py, checked without a device by
tests/test_marl_opts_cpu.py) on that test's fixture, bit for bit, and against the two existing
samplers at n_step = 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import marl_opts_util as mu
from replay_util import OBS_WORDS, SENTINEL
from test_replay_gpu import _bits, _device_ring, _need_gpu

pytestmark = pytest.mark.gpu

OUT_KEYS = ("s", "s2", "a", "r", "done", "gamma_row", "len", "idx")
FILL = dict(SENTINEL, gamma_row=np.float32(-3.5), len=-11, idx=-9)
PAST = 3  # rows behind the batch that must keep their sentinel


def _out(rows):
    n = rows + PAST
    i32, dev = torch.int32, "cuda"
    return dict(s=torch.full((n * OBS_WORDS,), FILL["s"], dtype=i32, device=dev),
                s2=torch.full((n * OBS_WORDS,), FILL["s2"], dtype=i32, device=dev),
                a=torch.full((n,), FILL["a"], dtype=i32, device=dev),
                r=torch.full((n,), float(FILL["r"]), dtype=torch.float32, device=dev),
                done=torch.full((n,), FILL["done"], dtype=torch.uint8, device=dev),
                gamma_row=torch.full((n,), float(FILL["gamma_row"]), dtype=torch.float32, device=dev),
                len=torch.full((n,), FILL["len"], dtype=i32, device=dev),
                idx=torch.full((n,), FILL["idx"], dtype=torch.int64, device=dev))


def _sample(rp, B, nets, joint, base, count, stride, n_step, gamma, out, optional=True):
    from evacx._lib import lib
    L = lib()
    rc = L.evx_replay_sample_nstep_agents(
        C.byref(rp.c), rp.size, B, nets, joint, mu.SEED, mu.OFFSET, base, count, stride, n_step, gamma,
        out["s"].data_ptr(), out["s2"].data_ptr(), out["a"].data_ptr(), out["r"].data_ptr(), out["done"].data_ptr(),
        out["gamma_row"].data_ptr(), out["len"].data_ptr() if optional else None,
        out["idx"].data_ptr() if optional else None, None)
    torch.cuda.synchronize()
    assert rc == 0, L.evx_q_last_error()


def _assert_rows(out, want, rows, what, keys=OUT_KEYS):
    for k in keys:
        per = OBS_WORDS if k in ("s", "s2") else 1
        got = out[k].cpu().numpy()
        assert np.array_equal(_bits(got[:rows * per]), _bits(want[k])), (what, k)
        assert np.all(got[rows * per:] == FILL[k]), (what, k, "rows past the batch")


@pytest.mark.parametrize("joint", [0, 1], ids=["agents", "joint"])
@pytest.mark.parametrize("state", mu.STATES)
@pytest.mark.parametrize("nets", mu.NETS)
def test_sampler_matches_the_restatement(nets, state, joint):
    """Every agent's whole population (B = size / nets: each of its slots once) at every n_step of
    the fixture: s, a, s2, r, done, gamma_row, len and idx_out bit for bit, nothing behind the batch
    written; len and idx_out NULL change nothing else. Joint mode: the agents' rows of a draw have
    equal len, r and done."""
    _need_gpu()
    ring = mu.ring_fixture(nets, state)
    rp = _device_ring(ring)
    base, count = ring.live_range()
    assert (base, count) == rp.live_range()
    stride, B = mu.stride_of(nets), ring.size // nets
    for n in mu.NSTEPS:
        want = mu.np_sample_nstep_agents(ring, B, nets, joint, mu.SEED, mu.OFFSET, base, count, stride, n, 0.99)
        out = _out(nets * B)
        _sample(rp, B, nets, joint, base, count, stride, n, 0.99, out)
        _assert_rows(out, want, nets * B, (state, n))
        bare = _out(nets * B)
        _sample(rp, B, nets, joint, base, count, stride, n, 0.99, bare, optional=False)
        _assert_rows(bare, want, nets * B, (state, n, "len / idx_out NULL"), OUT_KEYS[:6])
        assert bool((bare["len"] == FILL["len"]).all()) and bool((bare["idx"] == FILL["idx"]).all())
        if joint:
            for k in ("len", "r", "done"):
                rows = out[k][:nets * B].view(nets, B)
                assert bool((rows == rows[0]).all()), (state, n, k)
    # a stride beyond the ring stands for the capacity: no successor, every chain is one slot
    want = mu.np_sample_nstep_agents(ring, B, nets, joint, mu.SEED, mu.OFFSET, base, count, 1 << 40, 5, 0.99)
    assert (want["len"] == 1).all()
    out = _out(nets * B)
    _sample(rp, B, nets, joint, base, count, 1 << 40, 5, 0.99, out)
    _assert_rows(out, want, nets * B, (state, "stride beyond the ring"))


@pytest.mark.parametrize("joint", [0, 1], ids=["agents", "joint"])
@pytest.mark.parametrize("nets", mu.NETS)
def test_one_step_equals_the_existing_samplers(nets, joint):
    """n_step = 1: the s / s2 / a / r / done of evx_replay_sample_agents / _joint with the same
    (size, B, nets, seed, offset), bit for bit; gamma_row = gamma and len = 1. A smaller, odd B too."""
    _need_gpu()
    from evacx._lib import lib
    L = lib()
    for state in mu.STATES:
        ring = mu.ring_fixture(nets, state)
        rp = _device_ring(ring)
        base, count = ring.live_range()
        for B in (ring.size // nets, 5):
            out = _out(nets * B)
            _sample(rp, B, nets, joint, base, count, mu.stride_of(nets), 1, 0.97, out)
            old = _out(nets * B)
            fn = L.evx_replay_sample_joint if joint else L.evx_replay_sample_agents
            rc = fn(C.byref(rp.c), rp.size, B, nets, mu.SEED, mu.OFFSET, old["s"].data_ptr(), old["s2"].data_ptr(),
                    old["a"].data_ptr(), old["r"].data_ptr(), old["done"].data_ptr(), None)
            torch.cuda.synchronize()
            assert rc == 0, L.evx_q_last_error()
            for k in ("s", "s2", "a", "r", "done"):
                assert torch.equal(out[k], old[k]), (state, B, k)
            assert bool((out["gamma_row"][:nets * B] == np.float32(0.97)).all())
            assert bool((out["len"][:nets * B] == 1).all())
