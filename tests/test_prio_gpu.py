"""GPU prioritized replay (csrc/prio.hip) against the oracle (oracle/prio_oracle.c).

Trees are compared bit for bit (every internal node is left + right / min of its
children, so they are a pure function of the leaves); leaf priorities (td + eps)^alpha
come from the device pow and the C library pow, compared within 1 ulp, after which the
oracle adopts the GPU's leaves. Sample indices are exact; importance weights within one
float32 ulp (pow again).

The sampler is also held by a reference that is no tree (prio_util.cumsum_sample: a search in
the cumulative sum of exact leaves), and the range, update and argument edges of the kernels
by the oracle from saved random leaves: see the second half of this file."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from prio_util import PATTERNS, _adopt_leaves, check_sample, exact_td, leaf_patterns

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ring(C):
    from evacx.prio import PrioReplay
    rp = PrioReplay(C, "cuda")
    # distinct payloads so gathers can be checked: action = slot, reward = slot / 2
    rp.a.copy_(torch.arange(C, dtype=torch.int32, device="cuda"))
    rp.r.copy_(torch.arange(C, dtype=torch.float32, device="cuda") * 0.5)
    rp.s.view(C, -1)[:, 0] = torch.arange(C, dtype=torch.int32, device="cuda")
    return rp


@pytest.mark.parametrize("C", [1024, 1 << 15, 1 << 20, 1 << 22])  # 2^22: cfg5's ring, a three-pass rebuild
def test_trees_and_sampling_vs_oracle(C):
    _need_gpu()
    rp = _ring(C)
    o = orc.PrioTrees(C)
    rng = np.random.RandomState(C & 0xFFFF)
    from evacx.env import OBS_WORDS
    B = 4096
    out = dict(s=torch.zeros(B * OBS_WORDS, dtype=torch.int32, device="cuda"),
               s2=torch.zeros(B * OBS_WORDS, dtype=torch.int32, device="cuda"),
               a=torch.zeros(B, dtype=torch.int32, device="cuda"), r=torch.zeros(B, device="cuda"),
               done=torch.zeros(B, dtype=torch.uint8, device="cuda"))
    idx = torch.zeros(B, dtype=torch.int64, device="cuda")
    w = torch.zeros(B, device="cuda")
    pos = C - C // 3  # ranges wrap
    for it in range(6):
        n_new = int(rng.randint(1, C // 2))
        n_hide = int(rng.randint(0, C // 4)) if it % 2 else 0
        rp.pos, rp.unexposed = (pos + n_new) % C, n_new
        rp.expose(n_hide=n_hide)
        o.set_range(pos, n_new, n_hide)
        pos = (pos + n_new) % C
        torch.cuda.synchronize()
        assert np.array_equal(rp.tsum.cpu().numpy()[1:], o.sum[1:]), (it, "sum after set_range")
        assert np.array_equal(rp.tmin.cpu().numpy()[1:], o.mn[1:]), (it, "min after set_range")
        assert rp.max_leaf.item() == o.max_leaf[0]
        beta = 0.4 + 0.1 * it
        rp.sample_prio(B, beta, 99, it * B, out, idx, w)
        oi, ow = o.sample(B, beta, 99, it * B)
        gi = idx.cpu().numpy()
        assert np.array_equal(gi, oi), (it, "indices")
        gw = w.cpu().numpy()
        assert np.all(np.abs(gw - ow) <= np.spacing(ow)), (it, "weights")
        assert np.array_equal(out["a"].cpu().numpy(), oi.astype(np.int32))
        assert np.array_equal(out["r"].cpu().numpy(), (oi * 0.5).astype(np.float32))
        assert np.array_equal(out["s"].view(B, -1)[:, 0].cpu().numpy(), oi.astype(np.int32))
        assert np.all(o.sum[C + oi] > 0)  # never an empty or hidden slot
        # priorities of the sampled slots from TD errors, duplicates included
        td = (rng.rand(B) * 3).astype(np.float32)
        td_t = torch.from_numpy(td).cuda()
        rp.update(idx, td_t, B)
        o.update(oi, td, rp.eps, rp.alpha)
        torch.cuda.synchronize()
        _adopt_leaves(o, rp)


def test_trainer_prioritized_strict_and_lagged():
    _need_gpu()
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    from evacx.trainer import VecTrainer
    lay = DeviceLayout(build_tables(synthetic(64, 64, 8)), 569)
    for lagged in (False, True):
        tr = VecTrainer(lay, 64, batch=256, replay_capacity=1 << 12, lagged_learn=lagged, replay="prioritized")
        for _ in range(30):
            tr.step()
        tr.sync()
        torch.cuda.synchronize()
        assert tr.learn_steps > 0
        assert np.isfinite(tr.last_loss.item())
        C = tr.replay.capacity
        s = tr.replay.tsum.cpu().numpy()
        o = orc.PrioTrees(C)
        o.sum[:] = s
        o.mn[:] = tr.replay.tmin.cpu().numpy()
        o.set_range(0, 0, 0)
        assert np.array_equal(o.sum, s)  # internal nodes consistent with the leaves
        if lagged:  # the slots the next push overwrites are hidden
            hid = (tr.replay.pos - tr.n_agents + np.arange(tr.n_agents)) % C  # push t's slots
            assert np.all(s[C + hid] == 0)
        w = tr.samp["w"].cpu().numpy()
        assert np.all(w > 0) and np.all(w <= 1.0)


# ------------------------------------------------------------------ the sampler against a plain reference
def _random_ring(C, alpha=0.6, eps=1e-6):
    """A ring whose every word is random, so a gather of the wrong slot or field shows."""
    from evacx.prio import PrioReplay
    rp = PrioReplay(C, "cuda", alpha=alpha, eps=eps)
    g = torch.Generator(device="cuda").manual_seed(C)
    rp.s.copy_(torch.randint(-2**31, 2**31 - 1, rp.s.shape, device="cuda", generator=g, dtype=torch.int32))
    rp.s2.copy_(torch.randint(-2**31, 2**31 - 1, rp.s2.shape, device="cuda", generator=g, dtype=torch.int32))
    rp.a.copy_(torch.randint(-2**31, 2**31 - 1, rp.a.shape, device="cuda", generator=g, dtype=torch.int32))
    rp.r.copy_(torch.randn(C, device="cuda", generator=g))
    rp.done.copy_((torch.rand(C, device="cuda", generator=g) < 0.5).to(torch.uint8))
    return rp


def _outs(B):
    from evacx.env import OBS_WORDS
    return dict(s=torch.zeros(B * OBS_WORDS, dtype=torch.int32, device="cuda"),
                s2=torch.zeros(B * OBS_WORDS, dtype=torch.int32, device="cuda"),
                a=torch.zeros(B, dtype=torch.int32, device="cuda"), r=torch.zeros(B, device="cuda"),
                done=torch.zeros(B, dtype=torch.uint8, device="cuda"))


def _assert_rows(rp, out, j, B):
    """out's first B rows are the ring's rows at slots j (int64 device tensor)."""
    C = rp.capacity
    for k in ("s", "s2", "a", "r", "done"):
        got, ring = out[k].view(out["a"].numel(), -1)[:B], getattr(rp, k).view(C, -1)
        assert torch.equal(got.view(torch.uint8), ring[j].view(torch.uint8)), k  # byte for byte


def _set_range(rp, pos, n_new, n_hide):
    import ctypes as C
    from evacx._lib import check, lib
    check(lib().evx_prio_set_range(C.byref(rp.t), pos, n_new, n_hide, None), "prio_set_range")


def _exact_leaves(rp, o, slots, td):
    """Exact leaves td = m / 1024 at the slots, nothing elsewhere, on the device and the oracle.
    -> the leaf vector (float64 [C]).

    The oracle gets them through the public entry points (everything hidden, then update with
    eps = 0, alpha = 1: the C library's pow(x, 1.0) is x). The device's pow is within 1 ulp of x
    but not always x, and a leaf 1 ulp off a multiple of 2^-10 would void the exactness the
    reference rests on. So the device's update is held to the 1-ulp bar of the other tests, then
    the exact values are written over its leaves and the trees rebuilt by an update of the first
    slot with td = 1 (pow(1, 1) = 1 on the device, asserted)."""
    C = rp.capacity
    _set_range(rp, 0, 0, C)
    o.set_range(0, 0, C)
    rp.update(torch.from_numpy(slots).cuda(), torch.from_numpy(td).cuda(), len(slots))
    o.update(slots, td, 0.0, 1.0)
    p = np.zeros(C, np.float64)
    p[slots] = td.astype(np.float64)
    assert np.array_equal(o.sum[C:], p)
    torch.cuda.synchronize()
    got = rp.tsum.cpu().numpy()[C:]
    assert np.all(np.abs(got - p) <= np.spacing(p)) and np.array_equal(got == 0, p == 0)
    assert np.array_equal(rp.tmin.cpu().numpy()[C:][slots], got[slots])
    assert int((rp.owner != -1).sum()) == 0
    p[slots[0]] = 1.0
    exact = torch.from_numpy(p).cuda()
    rp.tsum[C:] = exact
    rp.tmin[C:] = torch.where(exact > 0, exact, torch.full_like(exact, float("inf")))
    rp.update(torch.from_numpy(slots[:1]).cuda(), torch.ones(1, device="cuda"), 1)
    o.update(slots[:1], np.ones(1, np.float32), 0.0, 1.0)
    torch.cuda.synchronize()
    assert np.array_equal(rp.tsum.cpu().numpy()[C:], p), "pow(1, 1) on the device is not 1"
    assert np.array_equal(rp.tsum.cpu().numpy()[1:], o.sum[1:]) and np.array_equal(rp.tmin.cpu().numpy()[1:], o.mn[1:])
    return p


SAMPLE_B = (1, 255, 257, 4096)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("C", [1024, 2048, 1 << 15])
def test_sampler_vs_cumulative_sum(C, pattern):
    """Exact leaves (multiples of 2^-10 below 64): the device's descent must pick the slots of
    searchsorted(cumsum(p), u) -- no tree, no shared code -- and the oracle's; B off the 256-thread
    block, a single row, fewer live leaves than rows, leaves at the ends and at a block boundary."""
    _need_gpu()
    rp = _random_ring(C, alpha=1.0, eps=0.0)
    o = orc.PrioTrees(C)
    rng = np.random.RandomState(C + 7)
    slots = leaf_patterns(C, rng)[pattern]
    p = _exact_leaves(rp, o, slots, exact_td(rng, len(slots)))
    out = _outs(max(SAMPLE_B))
    idx = torch.zeros(max(SAMPLE_B), dtype=torch.int64, device="cuda")
    w = torch.zeros(max(SAMPLE_B), device="cuda")
    for B in SAMPLE_B:
        for beta in (0.0, 0.4, 1.0):
            seed, offset = 23, 5 * B
            idx.fill_(-1)
            w.fill_(-1.0)
            rp.sample_prio(B, beta, seed, offset, out, idx, w)
            torch.cuda.synchronize()
            gi, gw = idx.cpu().numpy(), w.cpu().numpy()
            assert np.all(gi[B:] == -1) and np.all(gw[B:] == -1.0)  # nothing past row B
            check_sample(p, gi[:B], gw[:B], B, beta, seed, offset, what=(C, pattern, B, beta))
            oi, ow = o.sample(B, beta, seed, offset)
            assert np.array_equal(gi[:B], oi)
            assert np.all(np.abs(gw[:B] - ow) <= np.spacing(ow))
            _assert_rows(rp, out, idx[:B], B)


def test_sampler_without_index_and_weight_outputs():
    """evx_prio_sample with idx_out = w_out = NULL gathers the same rows."""
    _need_gpu()
    import ctypes as Ct
    from evacx._lib import check, lib
    C, B = 2048, 257
    rp = _random_ring(C, alpha=1.0, eps=0.0)
    o = orc.PrioTrees(C)
    rng = np.random.RandomState(3)
    slots = leaf_patterns(C, rng)["random37"]
    _exact_leaves(rp, o, slots, exact_td(rng, len(slots)))
    out = _outs(B)
    check(lib().evx_prio_sample(Ct.byref(rp.c), Ct.byref(rp.t), B, 0.4, 23, 77, out["s"].data_ptr(),
                                out["s2"].data_ptr(), out["a"].data_ptr(), out["r"].data_ptr(),
                                out["done"].data_ptr(), None, None, None), "prio_sample")
    torch.cuda.synchronize()
    oi, _ = o.sample(B, 0.4, 23, 77)
    _assert_rows(rp, out, torch.from_numpy(oi).cuda(), B)


# ------------------------------------------------------------------ range and update edges
EDGE_C = [1024, 2048, 1 << 21]  # one pass; a second pass over a 2-node block; three passes, 2 blocks in the middle


class _Edge:
    """A device tree and the oracle on the same non-trivial random leaves, restorable."""

    def __init__(self, C):
        from evacx.prio import PrioReplay
        self.C = C
        self.rp = PrioReplay(C, "cuda")
        self.o = orc.PrioTrees(C)
        rng = np.random.RandomState(C % 1000 + 1)
        self.rng = rng
        # slots C/8 .. 7C/8 live, the next C/16 hidden, then random priorities on up to half of the live slots
        self.rp.pos, self.rp.unexposed = (C // 8 + 3 * C // 4) % C, 3 * C // 4
        self.rp.expose(n_hide=C // 16)
        self.o.set_range(C // 8, 3 * C // 4, C // 16)
        live = (C // 8 + np.arange(3 * C // 4, dtype=np.int64)) % C
        n = min(len(live) // 2, 1 << 16)
        idx = rng.choice(live, n, replace=True)
        td = (rng.rand(n) * 3).astype(np.float32)
        self.update(idx, td)
        self.check_update()
        self.saved = (self.rp.tsum.clone(), self.rp.tmin.clone(), self.rp.max_leaf.clone(),
                      self.o.sum.copy(), self.o.mn.copy(), self.o.max_leaf.copy())

    def restore(self):
        s = self.saved
        self.rp.tsum.copy_(s[0])
        self.rp.tmin.copy_(s[1])
        self.rp.max_leaf.copy_(s[2])
        self.o.sum[:], self.o.mn[:], self.o.max_leaf[:] = s[3], s[4], s[5]

    def update(self, idx, td):
        idx, td = np.asarray(idx, np.int64), np.asarray(td, np.float32)
        self.rp.update(torch.from_numpy(idx).cuda(), torch.from_numpy(td).cuda(), len(idx))
        self.o.update(idx, td, self.rp.eps, self.rp.alpha)

    def check_update(self):
        """max_leaf within 1 ulp (the device pow against the C library's, as the leaves), leaves within
        1 ulp, then both trees bit for bit; owner all -1 again."""
        torch.cuda.synchronize()
        gmax, omax = self.rp.max_leaf.item(), self.o.max_leaf[0]
        assert abs(gmax - omax) <= np.spacing(omax), ("max_leaf", gmax, omax)
        _adopt_leaves(self.o, self.rp)
        assert int((self.rp.owner != -1).sum()) == 0, "owner not reset"

    def check_exact(self, what):
        torch.cuda.synchronize()
        assert np.array_equal(self.rp.tsum.cpu().numpy()[1:], self.o.sum[1:]), (what, "sum tree")
        assert np.array_equal(self.rp.tmin.cpu().numpy()[1:], self.o.mn[1:]), (what, "min tree")
        assert self.rp.max_leaf.item() == self.o.max_leaf[0], (what, "max_leaf")


@pytest.mark.parametrize("C", EDGE_C)
def test_set_range_edges_vs_oracle(C):
    _need_gpu()
    e = _Edge(C)
    cases = [(0, 1, 0), (C - 1, 2, 0), (1023, 1, 1), (1024, 1024, 0), (5, C, 0), (5, C - 7, 7), (0, 0, 3),
             (C - 3, 0, 6)]
    for pos, n_new, n_hide in cases:
        e.restore()
        _set_range(e.rp, pos, n_new, n_hide)
        e.o.set_range(pos, n_new, n_hide)
        e.check_exact((pos, n_new, n_hide))
        # and what the range means, not only that two restatements agree
        ls, lm = e.rp.tsum[C:], e.rp.tmin[C:]
        new = (pos + torch.arange(n_new, device="cuda")) % C
        hid = (pos + n_new + torch.arange(n_hide, device="cuda")) % C
        mx = e.saved[2].item()
        assert bool((ls[new] == mx).all()) and bool((lm[new] == mx).all())
        assert bool((ls[hid] == 0).all()) and bool(torch.isinf(lm[hid]).all())
        rest = torch.ones(C, dtype=torch.bool, device="cuda")
        rest[new] = False
        rest[hid] = False
        assert torch.equal(ls[rest], e.saved[0][C:][rest]) and torch.equal(lm[rest], e.saved[1][C:][rest])


@pytest.mark.parametrize("C", EDGE_C)
def test_update_edges_vs_oracle(C):
    _need_gpu()
    e = _Edge(C)
    rng, rp = e.rng, e.rp
    live = (C // 8 + np.arange(3 * C // 4, dtype=np.int64)) % C
    leaf = lambda j: rp.tsum[C + j].item()
    pw = lambda x: (float(np.float32(x)) + rp.eps) ** rp.alpha

    def near(a, b):
        return abs(a - b) <= np.spacing(b)

    # B = 1
    e.restore()
    e.update([live[5]], [2.5])
    e.check_update()
    assert near(leaf(live[5]), pw(2.5))
    # B = 257: one row past a 256-thread block
    e.restore()
    e.update(rng.choice(live, 257, replace=False), rng.rand(257) * 3)
    e.check_update()
    # 300 rows all naming one slot: the last row's value in the leaf, max_leaf the largest of all 300
    e.restore()
    td = (rng.rand(300) * 3).astype(np.float32)
    td[123], td[299] = 50.0, 0.125
    e.update(np.full(300, live[9]), td)
    e.check_update()
    assert near(leaf(live[9]), pw(0.125)) and near(rp.max_leaf.item(), pw(50.0))
    # td = 0: the leaf is eps ** alpha
    e.restore()
    e.update([live[0], live[1]], [0.0, 1.0])
    e.check_update()
    assert near(leaf(live[0]), rp.eps ** rp.alpha) and leaf(live[0]) > 0
    assert near(rp.tmin[1].item(), rp.eps ** rp.alpha)
    # td = 3e38: finite in the trees
    e.restore()
    e.update([live[2]], [3e38])
    e.check_update()
    assert near(leaf(live[2]), pw(3e38)) and np.isfinite(rp.tsum[1].item())
    assert near(rp.max_leaf.item(), pw(3e38))
    # two updates of one slot in a row, the second from a lower batch row than the first: the second wins
    e.restore()
    slot = live[77]
    e.update([live[3], live[4], live[6], slot], [0.5, 0.75, 1.0, 2.0])
    e.check_update()
    assert near(leaf(slot), pw(2.0))
    e.update([slot, live[8]], [0.25, 1.5])
    e.check_update()
    assert near(leaf(slot), pw(0.25)), "an update from a lower batch row was dropped (owner not reset)"


@pytest.mark.parametrize("C", EDGE_C)
def test_update_with_non_finite_td(C):
    """Rows whose priority is not finite change neither their slot's leaf nor max_leaf, yet own
    their slot when they are its last row (include/evacx.h): the trees stay finite and the
    oracle's, pinned by hand in tests/test_prio_cpu.py."""
    _need_gpu()
    e = _Edge(C)
    rng, rp = e.rng, e.rp
    live = (C // 8 + np.arange(3 * C // 4, dtype=np.int64)) % C
    sl = rng.choice(live, 6, replace=False)
    nan, inf = np.nan, np.inf
    idx = [sl[0], sl[1], sl[2], sl[0], sl[3], sl[4], sl[1], sl[4], sl[5], sl[4], sl[5]]
    td = [9.0, nan, inf, nan, 2.0, 1.0, 0.5, inf, nan, 0.25, nan]
    before = rp.tsum[C + torch.from_numpy(sl).cuda()].cpu().numpy()
    max0 = rp.max_leaf.item()
    assert max0 < (9.0 + rp.eps) ** rp.alpha
    e.update(idx, td)
    e.check_update()
    after = rp.tsum[C + torch.from_numpy(sl).cuda()].cpu().numpy()
    assert after[0] == before[0] and after[2] == before[2] and after[5] == before[5]  # last row not finite: kept
    near = lambda a, b: abs(a - b) <= np.spacing(b)
    pw = lambda x: (float(np.float32(x)) + rp.eps) ** rp.alpha
    assert near(after[1], pw(0.5)) and near(after[3], pw(2.0)) and near(after[4], pw(0.25))
    assert near(rp.max_leaf.item(), pw(9.0))  # the largest finite row, not +inf, not NaN
    assert bool(torch.isfinite(rp.tsum).all()) and not bool(torch.isnan(rp.tmin).any())
    # only non-finite rows: nothing changes at all
    t0, m0, x0 = rp.tsum.clone(), rp.tmin.clone(), rp.max_leaf.item()
    e.update([sl[0], sl[1], sl[1]], [nan, inf, nan])
    e.check_update()
    assert torch.equal(rp.tsum, t0) and torch.equal(rp.tmin, m0) and rp.max_leaf.item() == x0
    # a later push takes a finite max priority
    rp.pos, rp.unexposed = 7, 7
    rp.expose()
    e.o.set_range(0, 7, 0)
    e.check_exact("push after non-finite rows")
    assert bool((rp.tsum[C:C + 7] == x0).all())
