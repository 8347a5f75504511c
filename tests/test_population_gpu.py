"""Population training on the GPU (evacx.population): the four device entries against
the single-net pieces they replace, bit for bit (torch.equal), and ``PopulationTrainer`` against
``pop_util.SlowPopulation`` -- the same K members stepped one by one with ``Learner``, ``Replay`` and
``MLPFast.act``. Shapes: grid 48, 300 people, R = 4 (tests/test_qgroup_gpu.py's ``_env_obs``)."""
import csv
import math
import os

import numpy as np
import pytest
import torch

import pop_util as pu

pytestmark = pytest.mark.gpu
SENT_Q, SENT_A = 7.0, -3


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ 1. the blocked grouped act
@pytest.mark.parametrize("n", [2, 62, 66, 128])
@pytest.mark.parametrize("K", [1, 3, 5])
def test_act_gb_equals_single_net_acts(K, n):
    """evx_qmlp_act_gb against K MLPFast.act calls on the row blocks (drop row0 = k n, act_offset + k n,
    epsilon[k]): Q and actions by torch.equal. n: below a 64-row tile, one pair short of it, one pair
    over it, two tiles. Epsilons (0, 1, 0.3) cycled; 8 sentinel rows behind the last block stay."""
    _need_gpu()
    from evacx._lib import FWD_ACT_GROUPED_BLOCKED
    from evacx.qgroup import GroupedLearner
    from evacx.qmlp import NACT
    lay, env = pu.small_env()
    assert env.E * pu.R >= K * n
    grp = GroupedLearner(K, seed=8)
    eps = [(0.0, 1.0, 0.3)[k % 3] for k in range(K)]
    tail = 8
    q = torch.full(((K * n + tail) * NACT,), SENT_Q, device="cuda")
    act = torch.full((K * n + tail,), SENT_A, dtype=torch.int32, device="cuda")
    plan = grp.act_blocks_plan(lay.c, env.obs, n, eps, actions=act, q=q, drop_stream=12)
    assert plan.route == FWD_ACT_GROUPED_BLOCKED and plan.drop_mode == 1
    grp.act_blocks(lay.c, env.obs, n, eps, actions=act, q=q, act_seed=9, act_offset=33, drop_stream=12)
    torch.cuda.synchronize()
    seen = set()
    for k in range(K):
        qk = torch.empty(n * NACT, device="cuda")
        ak = torch.empty(n, dtype=torch.int32, device="cuda")
        grp.fast.nets[k].act(lay.c, env.obs[k * n * 8:(k + 1) * n * 8], n, drop=(grp.seed, 12, 0.2, None, k * n), q=qk,
                             actions=ak, epsilon=eps[k], act_seed=9, act_offset=33 + k * n)
        torch.cuda.synchronize()
        assert torch.equal(q[k * n * NACT:(k + 1) * n * NACT], qk), k
        assert torch.equal(act[k * n:(k + 1) * n], ak), k
        seen.add(tuple(qk[:NACT].tolist()))
    assert len(seen) == K  # the nets really differ
    assert bool((q[K * n * NACT:] == SENT_Q).all()) and bool((act[K * n:] == SENT_A).all())


# ------------------------------------------------------------------ 2. Adam with a learning rate per net
def _adam_state(G, seed=40):
    """A GroupedLearner with drawn gradients, moments and the gradients' norm partials."""
    from evacx.qgroup import GroupedLearner
    from evacx.qmlp import MLPFast
    grp = GroupedLearner(G, seed=seed)
    g = torch.Generator().manual_seed(3)
    grp.gflat.copy_(torch.randn(G, grp.npar, generator=g) * 0.01)
    grp.m.copy_(torch.randn(G, grp.npar, generator=g) * 0.01)
    grp.v.copy_(torch.rand(G, grp.npar, generator=g) * 1e-4)
    for k in range(G):
        MLPFast.sumsq_parts(grp.gflat[k], grp._ss[k])
    grp.adam_step = 4
    return grp


def _adam_buffers(grp):
    out = dict(flat=grp.flat, g=grp.gflat, m=grp.m, v=grp.v, norm=grp.norm)
    out.update({name: grp.fast.bufs[name] for name in pu.OPERANDS})
    return out


def _assert_same(a, b, what):
    for name, x in _adam_buffers(a).items():
        y = _adam_buffers(b)[name]
        assert torch.equal(x, y), (what, name, int((x != y).sum()))


def test_adam_pack3_gl_equals_single_net_steps():
    """evx_qmlp_adam_pack3_gl against K evx_qmlp_adam_pack3 calls with lr[k]: parameters, clipped
    gradients, m, v, norm and all nine operand copies by torch.equal; equal lr: evx_qmlp_adam_pack3_g
    bit for bit; the member with lr = 0 keeps its parameters (its moments still move)."""
    _need_gpu()
    from evacx._lib import evx_adam
    G, lrs = 3, [1e-3, 0.0, 3e-4]
    a, b = _adam_state(G), _adam_state(G)
    p0 = a.flat.clone()
    assert torch.equal(a.gflat, b.gflat) and a.gflat.abs().max().item() > 0
    a.step_optimizer(lr=lrs)
    b.adam_step += 1
    for k in range(G):
        h = evx_adam(lr=lrs[k], beta1=b.betas[0], beta2=b.betas[1], eps=b.eps, weight_decay=0.0, step=b.adam_step)
        b.fast.nets[k].adam_step(b.flat[k], b.gflat[k], b.m[k], b.v[k], float(b.max_norm), h, b._ss[k], b.norm[k:k + 1])
    torch.cuda.synchronize()
    _assert_same(a, b, "per-net lr")
    assert torch.equal(a.flat[1], p0[1]) and not torch.equal(a.flat[0], p0[0]) and not torch.equal(a.flat[2], p0[2])
    assert not torch.equal(a.m[1], _adam_state(G).m[1])
    c, d = _adam_state(G), _adam_state(G)
    c.lr = 3e-4
    c.step_optimizer()
    d.step_optimizer(lr=[3e-4] * G)
    torch.cuda.synchronize()
    _assert_same(c, d, "equal lr")
    with pytest.raises(ValueError):
        d.step_optimizer(lr=[1e-3])


# ------------------------------------------------------------------ 3. the replay rings
GUARD = 16  # slots / rows behind every array that must keep their sentinel


def _guarded_rings(K, cap):
    """A BlockReplay whose arrays are followed by GUARD sentinel slots."""
    from evacx._lib import evx_replay
    from evacx.population import BlockReplay
    br = BlockReplay(K, cap, "cuda")
    n = K * cap + GUARD
    br.s = torch.full((n * 8,), -5, dtype=torch.int32, device="cuda")
    br.s2 = torch.full((n * 8,), -6, dtype=torch.int32, device="cuda")
    br.a = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    br.r = torch.full((n,), -8.0, device="cuda")
    br.done = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    br.c = evx_replay(capacity=cap, s=br.s.data_ptr(), s2=br.s2.data_ptr(), a=br.a.data_ptr(), r=br.r.data_ptr(),
                      done=br.done.data_ptr())
    return br


@pytest.mark.parametrize("cap", [512, 600])
def test_replay_blocks_equal_separate_rings(cap):
    """evx_replay_push_blocks / evx_replay_sample_blocks against K Replay rings pushed and sampled one
    by one: N = 128 rows per ring and push. cap 512: N divides it; 600: the fifth push straddles the
    wrap. Sampled (B = 190 and 256) before the rings are full and after they wrap; every ring array
    and every sampled array by torch.equal; the sentinels behind ring K - 1 and behind the outputs stay."""
    _need_gpu()
    from evacx.trainer import Replay
    K, N, R = 3, 128, 4
    br = _guarded_rings(K, cap)
    seps = [Replay(cap, "cuda") for _ in range(K)]
    for rp in seps:  # the same fill as the guarded rings' unwritten slots
        rp.s.fill_(-5), rp.s2.fill_(-6), rp.a.fill_(-7), rp.r.fill_(-8.0), rp.done.fill_(9)
    g = torch.Generator().manual_seed(cap)
    draws = 0

    def push():
        s = torch.randint(0, 1 << 30, (K * N * 8,), generator=g, dtype=torch.int32).cuda()
        s2 = torch.randint(0, 1 << 30, (K * N * 8,), generator=g, dtype=torch.int32).cuda()
        st = torch.randint(0, 1 << 30, (K * N * 8,), generator=g, dtype=torch.int32).cuda()
        a = torch.randint(0, 5, (K * N,), generator=g, dtype=torch.int32).cuda()
        r = (torch.randn(K * N // R, generator=g, dtype=torch.float64) * 30).cuda()
        d = (torch.rand(K * N // R, generator=g) < 0.3).to(torch.uint8).cuda()
        assert 0 < int(d.sum()) < d.numel()
        br.push(s, s2, a, r, d, N, R, s2_term=st)
        for k, rp in enumerate(seps):
            rows, envs = slice(k * N * 8, (k + 1) * N * 8), slice(k * N // R, (k + 1) * N // R)
            rp.push(s[rows], s2[rows], a[k * N:(k + 1) * N], r[envs], d[envs], N, R, s2_term=st[rows])
        torch.cuda.synchronize()
        assert (br.pos, br.size) == (seps[0].pos, seps[0].size)
        for name, per, sent in (("s", 8, -5), ("s2", 8, -6), ("a", 1, -7), ("r", 1, -8.0), ("done", 1, 9)):
            arr = getattr(br, name)
            for k, rp in enumerate(seps):
                assert torch.equal(arr[k * cap * per:(k + 1) * cap * per], getattr(rp, name)), (name, k, br.pos)
            tail = arr[K * cap * per:]
            assert tail.numel() == GUARD * per and bool((tail == sent).all()), name

    def sample(B):
        nonlocal draws
        out = dict(s=torch.full(((K * B + GUARD) * 8,), -1, dtype=torch.int32, device="cuda"),
                   s2=torch.full(((K * B + GUARD) * 8,), -1, dtype=torch.int32, device="cuda"),
                   a=torch.full((K * B + GUARD,), -1, dtype=torch.int32, device="cuda"),
                   r=torch.full((K * B + GUARD,), -1.0, device="cuda"),
                   done=torch.full((K * B + GUARD,), 7, dtype=torch.uint8, device="cuda"))
        br.sample(B, 18, draws * K * B, out)
        for k, rp in enumerate(seps):
            o = dict(s=torch.zeros(B * 8, dtype=torch.int32, device="cuda"),
                     s2=torch.zeros(B * 8, dtype=torch.int32, device="cuda"),
                     a=torch.zeros(B, dtype=torch.int32, device="cuda"), r=torch.zeros(B, device="cuda"),
                     done=torch.zeros(B, dtype=torch.uint8, device="cuda"))
            rp.sample(B, 18, (draws * K + k) * B, o)
            torch.cuda.synchronize()
            for name, per in (("s", 8), ("s2", 8), ("a", 1), ("r", 1), ("done", 1)):
                assert torch.equal(out[name][k * B * per:(k + 1) * B * per], o[name]), (name, k, B)
        for name, per, v in (("s", 8, -1), ("s2", 8, -1), ("a", 1, -1), ("r", 1, -1.0), ("done", 1, 7)):
            assert bool((out[name][K * B * per:] == v).all()), name
        assert not torch.equal(out["a"][:B], out["a"][B:2 * B]) or not torch.equal(out["r"][:B], out["r"][B:2 * B])
        draws += 1

    push()
    push()  # size 256 of 512 / 600: not full
    for B in (190, 256):
        sample(B)
    for _ in range(4):  # cap 512: full after 4, wrapped after 6; cap 600: the fifth push straddles the end
        push()
    assert br.size == cap and br.pos == (6 * N) % cap
    for B in (190, 256):
        sample(B)


# ------------------------------------------------------------------ 4 - 8. the trainer
E, K, B, CAP, STEPS = 96, 3, 256, 1024, 12
HP = dict(lr=(1e-3, 3e-4, 1e-4), gamma=(0.99, 0.95, 0.9), epsilon=(1.0, 0.6, 0.3), epsilon_min=0.02,
          epsilon_decay=(0.9, 0.8, 0.95), target_every=(2, 3, 5))
_RUNS = {}


def _run(key, cls=None, stats=False, **over):
    """STEPS steps of a population (or of SlowPopulation), with the actions, reward, done, counts and
    losses of every step on the host: made once per key, shared by the tests below."""
    if key in _RUNS:
        return _RUNS[key]
    from evacx.population import PopulationTrainer
    hp = dict(HP)
    hp.update(over)
    kw = dict(episode_stats=True, learn_stats=True) if stats else {}
    tr = (cls or PopulationTrainer)(pu.small_layout(), E, members=K, seed=5, batch=B, replay_capacity=CAP, **hp, **kw)
    rec = dict(actions=[], reward=[], done=[], counts=[], loss=[])
    for _ in range(STEPS):
        tr.step()
        torch.cuda.synchronize()
        rec["actions"].append(tr.actions.cpu().clone())
        rec["reward"].append(tr.env.reward.cpu().clone())
        rec["done"].append(tr.env.done.cpu().clone())
        rec["counts"].append(tr.env.counts.cpu().clone())
        rec["loss"].append(None if tr.last_loss is None else tr.last_loss.cpu().clone())
    tr.env.check_err()
    _RUNS[key] = (tr, rec)
    return _RUNS[key]


def test_trainer_equals_slow_population():
    """K = 3, E = 96 (N = 128), B = 256, C = 1024, 12 steps (11 learn steps), lr, gamma, epsilon
    schedule and target period per member: actions, reward and done equal at every step; at the end the
    online and target parameters and m and v equal those of the K separate Learners (torch.equal); the
    loss to 1e-6 relative, the bar (and the reason) of
    tests/test_qgroup_gpu.py::test_grouped_learn_equals_separate_learners."""
    _need_gpu()
    pop, rp = _run("pop", stats=True)
    slow, rs = _run("slow", cls=pu.SlowPopulation)
    assert pop.learn_steps == slow.learn_steps == STEPS - 1
    for t in range(STEPS):
        for name in ("actions", "reward", "done"):
            assert torch.equal(rp[name][t], rs[name][t]), (t, name)
        if rs["loss"][t] is None:
            assert rp["loss"][t] is None
            continue
        for k in range(K):
            a, b = rp["loss"][t][k].item(), rs["loss"][t][k].item()
            print(f"step {t} member {k}: loss {a!r} slow {b!r}")
            assert abs(a - b) <= 1e-6 * abs(b), (t, k, a, b)
    gl = pop.glearner
    for k, lr in enumerate(slow.learners):
        assert torch.equal(gl.flat[k], lr.online.flat), k
        assert torch.equal(gl.tflat[k], lr.target.flat), k
        assert torch.equal(gl.m[k], lr.m) and torch.equal(gl.v[k], lr.v), k
        assert pop.epsilon[k] == slow.epsilon[k]
    assert len({tuple(a.tolist()) for a in rp["actions"]}) == STEPS
    # the target periods were honoured: member 0 synced at learn step 10, member 1 at 9, member 2 at 10
    assert not torch.equal(gl.tflat[1], gl.flat[1]) and not torch.equal(gl.tflat[0], gl.tflat[2])


def test_members_are_independent():
    """The same run with member 1's lr and exploration changed: members 0 and 2 keep their actions
    and parameters bit for bit, member 1 does not."""
    _need_gpu()
    pop, ra = _run("pop", stats=True)
    oth, rb = _run("other", lr=(1e-3, 5e-3, 1e-4), epsilon=(1.0, 0.1, 0.3))
    N = pop.N
    for t in range(STEPS):
        for k in (0, 2):
            assert torch.equal(ra["actions"][t][k * N:(k + 1) * N], rb["actions"][t][k * N:(k + 1) * N]), (t, k)
    for k in (0, 2):
        for name in ("flat", "tflat", "m", "v"):
            assert torch.equal(getattr(pop.glearner, name)[k], getattr(oth.glearner, name)[k]), (k, name)
    assert any(not torch.equal(ra["actions"][t][N:2 * N], rb["actions"][t][N:2 * N]) for t in range(STEPS))
    assert not torch.equal(pop.glearner.flat[1], oth.glearner.flat[1])


def test_two_equal_populations_are_bit_identical():
    _need_gpu()
    pop, ra = _run("pop", stats=True)
    two, rb = _run("again")  # (statistics off: they do not bear on the training)
    for t in range(STEPS):
        for name in ("actions", "reward", "done", "counts"):
            assert torch.equal(ra[name][t], rb[name][t]), (t, name)
        assert (ra["loss"][t] is None) == (rb["loss"][t] is None)
        if ra["loss"][t] is not None:
            assert torch.equal(ra["loss"][t], rb["loss"][t]), t
    for name in ("flat", "tflat", "m", "v", "gflat", "norm"):
        assert torch.equal(getattr(pop.glearner, name), getattr(two.glearner, name)), name
    for name in pu.OPERANDS:
        assert torch.equal(pop.glearner.fast.bufs[name], two.glearner.fast.bufs[name]), name
        assert torch.equal(pop.glearner.fast_t.bufs[name], two.glearner.fast_t.bufs[name]), name


def test_summaries_match_the_recorded_steps():
    """episode_summary()["per_member"] against a host accumulation of the recorded reward, done and
    counts over each member's envs (the episodes in progress too, per env, bit for bit);
    learn_summary() has K nets with finite values."""
    _need_gpu()
    pop, rec = _run("pop", stats=True)
    Ek, P = E // K, pu.PEOPLE
    ret, ln = np.zeros(E), np.zeros(E, np.int64)
    fin = [[] for _ in range(E)]  # (return, length, evacuated, dead) of every finished episode
    for t in range(STEPS):
        ret = ret + rec["reward"][t].numpy()
        ln += 1
        cnt = rec["counts"][t].numpy().reshape(E, 2)
        for e in np.nonzero(rec["done"][t].numpy())[0]:
            fin[e].append((ret[e], int(ln[e]), int(cnt[e, 0]), int(cnt[e, 1])))
            ret[e], ln[e] = 0.0, 0
    torch.cuda.synchronize()
    assert np.array_equal(pop.episodes.ret.cpu().numpy().view(np.int64), ret.view(np.int64))
    assert np.array_equal(pop.episodes.len.cpu().numpy(), ln)
    s = pop.episode_summary(clear=False)
    assert len(s["per_member"]) == K and "per_layout" not in s
    for k, row in enumerate(s["per_member"]):
        eps = [x for e in range(k * Ek, (k + 1) * Ek) for x in fin[e]]
        assert row["episodes"] == len(eps) and row["length_sum"] == sum(x[1] for x in eps)
        assert row["evacuated"] == sum(x[2] for x in eps) and row["dead"] == sum(x[3] for x in eps)
        ref = math.fsum(x[0] for x in eps)
        assert abs(row["return_sum"] - ref) <= 64 * 2.0 ** -52 * math.fsum(abs(x[0]) for x in eps)
        assert row["no_episode"] == sum(1 for e in range(k * Ek, (k + 1) * Ek) if not fin[e])
        if eps:
            assert row["evac_rate"] == row["evacuated"] / (len(eps) * P)
    assert s["episodes"] == sum(len(f) for f in fin)
    ls = pop.learn_summary(clear=False)
    assert len(ls["per_net"]) == K and ls["steps"] == STEPS - 1
    for k, net in enumerate(ls["per_net"]):
        assert net["steps"] == STEPS - 1 and net["rows"] == (STEPS - 1) * B and net["rows_bad"] == 0, k
        for name in ("q_mean", "target_mean", "td_abs_mean", "loss_mean", "grad_norm_mean"):
            assert net[name] is not None and math.isfinite(net[name]), (k, name)
    # the discount per member reached the statistics: member 2 (gamma 0.9) and member 0 (0.99) differ
    assert ls["per_net"][0]["target_mean"] != ls["per_net"][2]["target_mean"]
    from evacx.population import PopulationTrainer
    off = PopulationTrainer(pu.small_layout(), 8, members=2, batch=16, replay_capacity=64)
    with pytest.raises(RuntimeError):
        off.episode_summary()
    with pytest.raises(RuntimeError):
        off.learn_summary()


# ------------------------------------------------------------------ 7. members
def _small_pop(**kw):
    from evacx.population import PopulationTrainer
    args = dict(members=3, seed=2, batch=64, replay_capacity=256, lr=1e-3, epsilon=(0.5, 0.2, 0.0), epsilon_decay=1.0,
                target_every=4)
    args.update(kw)
    return PopulationTrainer(pu.small_layout(), 24, **args)


def test_copy_member_and_repack():
    _need_gpu()
    pop = _small_pop()
    for _ in range(5):
        pop.step()
    gl = pop.glearner
    assert not torch.equal(gl.flat[0], gl.flat[2]) and not torch.equal(gl.tflat[0], gl.tflat[2])
    keep = {name: getattr(gl, name)[1].clone() for name in ("flat", "tflat", "m", "v")}
    pop.copy_member(0, 2)
    torch.cuda.synchronize()
    for name in ("flat", "tflat", "m", "v"):
        assert torch.equal(getattr(gl, name)[2], getattr(gl, name)[0]), name
        assert torch.equal(getattr(gl, name)[1], keep[name]), name
    for fast in (gl.fast, gl.fast_t):
        got = {name: fast.bufs[name][2].clone() for name in pu.OPERANDS}
        for name in pu.OPERANDS:
            assert torch.equal(got[name], fast.bufs[name][0]), name
        fast.nets[2].repack()
        torch.cuda.synchronize()
        for name in pu.OPERANDS:
            assert torch.equal(got[name], fast.bufs[name][2]), name
    with pytest.raises(ValueError, match="3"):
        pop.copy_member(0, 3)
    pop.step()  # the copies now act and learn on their own envs and rings
    torch.cuda.synchronize()
    assert not torch.equal(gl.flat[2], gl.flat[0])


def test_set_hparams_takes_effect_at_the_next_step_only():
    """Two equal populations; one sets member 1's lr to 0, its gamma to 0.5 and its epsilon to 1 after
    step 3. Every member is equal up to there; at the next step members 0 and 2 stay equal bit for
    bit, member 1's parameters stand still (lr 0), its loss differs (gamma) and its actions differ
    (every one drawn). Bad values and names are refused."""
    _need_gpu()
    a, b = _small_pop(), _small_pop()
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.glearner.flat, b.glearner.flat) and torch.equal(a.actions, b.actions)
    b.set_hparams(1, lr=0.0, gamma=0.5, epsilon=1.0)
    assert b.lr == [1e-3, 0.0, 1e-3] and b.gamma[1] == 0.5 and a.lr[1] == 1e-3
    assert torch.equal(b.gamma_row.cpu(), torch.tensor([0.99] * 64 + [0.5] * 64 + [0.99] * 64))
    frozen = b.glearner.flat[1].clone()
    a.step()
    b.step()
    torch.cuda.synchronize()
    N = a.N
    for k in (0, 2):
        assert torch.equal(a.glearner.flat[k], b.glearner.flat[k]), k
        assert torch.equal(a.actions[k * N:(k + 1) * N], b.actions[k * N:(k + 1) * N]), k
    assert torch.equal(b.glearner.flat[1], frozen) and not torch.equal(a.glearner.flat[1], frozen)
    assert not torch.equal(a.actions[N:2 * N], b.actions[N:2 * N])  # epsilon 1: every action drawn
    assert a.glearner.loss[1].item() != b.glearner.loss[1].item()  # gamma entered the target
    for bad in (dict(lr=float("nan")), dict(gamma=1.5), dict(target_every=0), dict(momentum=0.9)):
        with pytest.raises(ValueError):
            b.set_hparams(0, **bad)
    with pytest.raises(ValueError):
        b.set_hparams(5, lr=1e-3)


def test_member_learner_and_checkpoint_round_trip(tmp_path):
    _need_gpu()
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(pu.__file__)), "..", "dqn-marl_amd"))
    from Louvre_Evacuation.runners.evaluate_vec import load_learner
    pop = _small_pop()
    for _ in range(5):
        pop.step()
    gl = pop.glearner
    for k in range(pop.K):
        lr = pop.member_learner(k)
        torch.cuda.synchronize()
        assert torch.equal(lr.online.flat, gl.flat[k]) and torch.equal(lr.target.flat, gl.tflat[k]), k
        assert torch.equal(lr.m, gl.m[k]) and torch.equal(lr.v, gl.v[k]) and lr.adam_step == gl.adam_step
        assert (lr.lr, lr.gamma) == (pop.lr[k], pop.gamma[k])
        for name in pu.OPERANDS:
            assert torch.equal(getattr(lr.fast, name), gl.fast.bufs[name][k]), (k, name)
            assert torch.equal(getattr(lr.fast_t, name), gl.fast_t.bufs[name][k]), (k, name)
        ck = pop.checkpoint(k)
        assert set(ck) == {"q_network", "target_network", "optimizer", "epsilon", "steps"}
        assert ck["steps"] == pop.learn_steps and ck["epsilon"] == pop.epsilon[k]
        assert ck["optimizer"]["param_groups"][0]["lr"] == pop.lr[k] and len(ck["optimizer"]["state"]) == 6
        path = tmp_path / f"m{k}.pth"
        torch.save(ck, path)
        back = load_learner(str(path), "cuda")
        torch.cuda.synchronize()
        assert torch.equal(back.online.flat, gl.flat[k]), k
        tgt = torch.cat([v.reshape(-1) for v in torch.load(path, weights_only=True)["target_network"].values()])
        assert torch.equal(tgt, gl.tflat[k].cpu()), k
    from evacx.evaluate import evaluate
    ev = evaluate(pu.small_layout(), 8, 1, "greedy", learner=pop.member_learner(0), seed=0)
    assert ev["episodes"] >= 1 and math.isfinite(ev["return_mean"])


# ------------------------------------------------------------------ 9. the runner
def test_train_pop_runner_writes_consistent_files(tmp_path):
    _need_gpu()
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(pu.__file__)), "..", "dqn-marl_amd"))
    from Louvre_Evacuation.runners import train_pop
    from Louvre_Evacuation.runners.evaluate_vec import load_learner
    cfg = tmp_path / "small.yaml"
    cfg.write_text("env:\n  width: 36\n  height: 30\n  fire_zones: [[18, 14]]\n  exit_location: [36, 15]\n"
                   "  num_people: 40\nagent:\n  gamma: 0.99\n  epsilon: 1.0\n  epsilon_min: 0.02\n"
                   "  epsilon_decay: 0.9995\n  learning_rate: 0.0001\n  batch_size: 32\n  target_update_freq: 20\n"
                   "  memory_size: 1024\nsave_path: \"unused\"\n")
    out = tmp_path / "out"
    tr = train_pop.main(["--config", str(cfg), "--members", "2", "--envs", "16", "--steps", "6", "--log-every", "3",
                         "--lr", "1e-3,1e-4", "--gamma", "0.9", "--seeds", "7,8", "--batch", "16", "--out", str(out)])
    assert tr.K == 2 and tr.lr == [1e-3, 1e-4] and tr.gamma == [0.9, 0.9] and tr.init_seeds == [7, 8]
    member_rows = []
    for k in range(2):
        rows = list(csv.reader(open(out / f"member{k}" / "training_log.csv")))
        assert rows[0] == train_pop.CSV_COLUMNS and [r[0] for r in rows[1:]] == ["3", "6"]
        member_rows.append(rows[1:])
        lr = load_learner(str(out / f"member{k}" / "dqn_model.pth"), "cuda")
        torch.cuda.synchronize()
        assert torch.equal(lr.online.flat, tr.glearner.flat[k]), k
    summ = list(csv.reader(open(out / "population_summary.csv")))
    assert summ[0] == train_pop.SUMMARY_COLUMNS and [r[0] for r in summ[1:]] == ["3", "6"]
    col = {name: i for i, name in enumerate(train_pop.CSV_COLUMNS)}
    scol = {name: i for i, name in enumerate(train_pop.SUMMARY_COLUMNS)}
    for i, srow in enumerate(summ[1:]):
        for key in ("reward", "evac_rate", "death_rate"):
            vals = [float(m[i][col[key]]) for m in member_rows if m[i][col[key]] != ""]
            if not vals:
                assert srow[scol[key + "_mean"]] == ""
                continue
            assert float(srow[scol[key + "_mean"]]) == pytest.approx(sum(vals) / len(vals), rel=1e-12, abs=1e-12)
            assert float(srow[scol[key + "_min"]]) == min(vals) and float(srow[scol[key + "_max"]]) == max(vals)
    import json
    best = json.load(open(out / "best_member.json"))
    assert best["member"] in (0, 1) and set(best) >= {"member", "death_rate", "evac_rate", "lr", "gamma", "seed"}
