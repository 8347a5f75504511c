"""The trainer's prioritized schedules (the self.prio branches of evacx/trainer.py) against a
host shadow: an oracle tree (oracle/prio_oracle.c) driven by a restatement of PrioReplay.push /
expose and of the two schedules of VecTrainer.step,

  strict: push, expose(), learn;
  lagged: expose(n_hide = n_agents), learn from the ring as it stood before this step's push.

After every step (synced) the learner's batch must be the shadow's sample -- the slots, the
annealed beta in the weights, the Philox offset learn_steps * batch --, the rows the ring's rows,
the loss mean(w td^2) of the device's own w and |TD|, and the trees the shadow's after it takes
that |TD| (leaves within 1 ulp: device pow against the C library's; then bit for bit). A second,
free-running trainer (no sync between steps) must end bit-identical to the synced one: the strict
schedule's priority update runs on its own stream beside clip + Adam and the next act / env.step
/ push, and a missing event wait can only show as a difference there."""
import functools

import numpy as np
import pytest
import torch

from prio_util import ShadowPrio, _adopt_leaves

pytestmark = pytest.mark.gpu

STEPS, E, BATCH, CAP, BETA_STEPS = 30, 64, 256, 1 << 12, 20

CASES = {
    "strict": dict(),
    "lagged": dict(lagged_learn=True),
    "groups2": dict(groups=2),
    "nstep3": dict(n_step=3),
    "exact": dict(precision="exact"),  # the dense path (evx_td_loss_w): fast is None, update on the main stream
    # lagged from step 10, strict again from step 20, each flip after a sync as bench.py's other
    # schedule (the act's and the expose's event waits of either schedule rest on that sync)
    "flip": dict(),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=1)
def _layout():
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables, synthetic
    return DeviceLayout(build_tables(synthetic(64, 64, 8)), 569)


def _trainer(replay="prioritized", **kw):
    from evacx.trainer import VecTrainer
    return VecTrainer(_layout(), E, batch=BATCH, replay_capacity=CAP, replay=replay, prio_beta_steps=BETA_STEPS,
                      target_every=5, lr=1e-3, **kw)


def _lagged_at(case, t, tr):
    if case == "flip":
        return 10 <= t < 20
    return tr.lagged


def _final_state(tr):
    """What a run leaves behind, on the host (after a sync)."""
    rp, ln = tr.replay, tr.learner
    st = {k: getattr(rp, k).cpu() for k in ("s", "s2", "a", "r", "done")}
    st.update(online=ln.online.flat.cpu(), target=ln.target.flat.cpu(), m=ln.m.cpu(), v=ln.v.cpu(),
              pos=rp.pos, learn_steps=tr.learn_steps)
    if tr.prio:
        st.update(tsum=rp.tsum.cpu(), tmin=rp.tmin.cpu(), max_leaf=rp.max_leaf.cpu(), owner=rp.owner.cpu(),
                  idx=tr.samp["idx"].cpu(), w=tr.samp["w"].cpu(), td=tr.samp["td"].cpu())
    return st


def _same(a, b):
    """Bit-identical tensors (NaNs included)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8).view(-1),
                                                                    b.contiguous().view(torch.uint8).view(-1))


@functools.lru_cache(maxsize=None)
def _synced_run(case):
    """The case's 30 steps, synced and checked against the shadow after every step. -> _final_state."""
    from evacx.env import OBS_WORDS
    tr = _trainer(**CASES[case])
    rp, n, C, B = tr.replay, tr.n_agents, CAP, BATCH
    assert n == 512 and rp.capacity == C and tr.prio
    if case == "exact":
        assert tr.fast is None and not tr.lagged
    sh = ShadowPrio(C)
    updated = set()   # slots whose leaf comes from a priority update
    watch = set()     # ... that a push then overwrote, waiting for their expose
    learned = wraps = max_hits = n_lagged = beta_one = 0
    for t in range(STEPS):
        if case == "flip":
            tr.lagged = 10 <= t < 20
        lag = tr.lagged
        ls0 = tr.learn_steps
        tr.step()
        tr.sync()
        torch.cuda.synchronize()
        # ---- the shadow's step, up to the sample
        if lag:
            n_lagged += 1
            win = sh.window(n)
            do = win[1] >= B
            newly = sh.expose(n_hide=n)
        else:
            pushed = sh.push(n)
            wraps += int(sh.pos < n)
            over = updated.intersection(pushed.tolist())
            watch |= over
            updated -= set(pushed.tolist())
            newly = sh.expose()
            do = sh.size >= B
        max_at_expose = sh.o.max_leaf[0]
        hit = watch.intersection(newly.tolist())
        watch -= hit
        assert tr.learn_steps == ls0 + int(do), (t, "a learn step more or less than the schedule's")
        leaves = rp.tsum[C:].cpu().numpy()
        if do:
            learned += 1
            beta = min(1.0, tr.prio_beta0 + (1.0 - tr.prio_beta0) * ls0 / BETA_STEPS)
            beta_one += int(beta == 1.0)
            oi, ow = sh.o.sample(B, beta, tr.seed + 1, ls0 * B)
            gi, gw = tr.samp["idx"].cpu().numpy(), tr.samp["w"].cpu().numpy()
            td = tr.samp["td"].cpu().numpy()
            assert np.array_equal(gi, oi), (t, "the learner trained on other slots than the trees prescribe")
            assert np.all(np.abs(gw - ow) <= np.spacing(ow)), (t, "weights", beta)
            j = tr.samp["idx"]
            rows = ("s", "a") if tr.n_step > 1 else ("s", "s2", "a", "r", "done")  # n-step rows replace r / done / s2
            for k in rows:
                w_ = OBS_WORDS if k in ("s", "s2") else 1
                assert torch.equal(tr.samp[k].view(B, w_), getattr(rp, k).view(C, w_)[j]), (t, k)
            # the importance weights reach the loss: B non-negative f32 terms and their sum
            want = float(np.mean(gw.astype(np.float64) * td.astype(np.float64) ** 2))
            got = float(tr.last_loss.item())
            print(f"{case} t={t} beta={beta:.3f} loss={got:.9g} ref={want:.9g} rel={abs(got - want) / want:.3g}")
            assert np.isfinite(td).all() and abs(got - want) <= 2 * B * 2.0 ** -24 * want, (t, got, want)
            sh.o.update(gi, td, rp.eps, rp.alpha)
            gmax, omax = rp.max_leaf.item(), sh.o.max_leaf[0]
            assert abs(gmax - omax) <= np.spacing(omax), (t, "max_leaf", gmax, omax)  # (a pow value, as the leaves)
            assert gmax >= max(max_at_expose, leaves[gi].max())
            updated |= set(gi.tolist())
        else:
            gi = np.zeros(0, np.int64)
            assert rp.max_leaf.item() == sh.o.max_leaf[0]
        # slots a push overwrote after an update hold the max priority of their expose
        keep = np.array(sorted(hit - set(gi.tolist())), np.int64)
        assert np.all(leaves[keep] == max_at_expose), (t, "overwritten slots without the max priority")
        max_hits += len(keep)
        if lag:  # this step's push: its slots were hidden from the learn step and still are
            pushed = sh.push(n)
            wraps += int(sh.pos < n)
            assert not np.isin(gi, pushed).any(), (t, "the lagged learn sampled a slot the running push writes")
            assert np.all(leaves[pushed] == 0) and bool(torch.isinf(rp.tmin[C:][torch.from_numpy(pushed).cuda()]).all())
            watch |= updated.intersection(pushed.tolist())
            updated -= set(pushed.tolist())
        assert rp.pos == sh.pos and rp.size == sh.size and rp.unexposed == sh.unexposed, t
        _adopt_leaves(sh.o, rp)
        assert rp.max_leaf.item() == sh.o.max_leaf[0]
        assert int((rp.owner != -1).sum()) == 0, (t, "owner not reset")
    # the run has what the checks are about
    assert learned >= 28 and wraps >= 3 and beta_one >= 5, (learned, wraps, beta_one)
    assert max_hits > 0, "no learn step's updated slots were overwritten by a later push"
    if case in ("lagged", "flip"):
        assert n_lagged == (STEPS if case == "lagged" else 10)
    return _final_state(tr)


@pytest.mark.parametrize("case", list(CASES))
def test_prioritized_schedule_vs_shadow(case):
    _need_gpu()
    _synced_run(case)


def _free_run(replay, case, synced):
    tr = _trainer(replay=replay, **CASES[case])
    for _ in range(STEPS):
        tr.step()
        if synced:
            tr.sync()
            torch.cuda.synchronize()
    tr.sync()
    torch.cuda.synchronize()
    return _final_state(tr)


@pytest.mark.parametrize("case", ["strict", "lagged", "groups2"])
def test_free_running_equals_synced(case):
    """30 steps with no sync between them end bit-identical to the run synced after every step:
    first the uniform replay (the control: nothing of the priority stream runs), then the
    prioritized one, whose synced run is the one checked against the shadow above."""
    _need_gpu()
    ctl_s, ctl_f = _free_run("uniform", case, True), _free_run("uniform", case, False)
    for k in ctl_s:
        same = _same(ctl_s[k], ctl_f[k]) if torch.is_tensor(ctl_s[k]) else ctl_s[k] == ctl_f[k]
        assert same, ("uniform control", k)
    ref, free = _synced_run(case), _free_run("prioritized", case, False)
    for k in ref:
        same = _same(ref[k], free[k]) if torch.is_tensor(ref[k]) else ref[k] == free[k]
        assert same, ("prioritized", k)
