"""evx_qmix_loss_opt alone (csrc/qmix.hip: the rows kernel with the TD options compiled in) against
MixingNetwork in float64 with autograd -- tests/test_qgroup_gpu.py's _mixer_reference extended by
sel (Double-Q), the Huber loss and gamma_row -- at that module's MIX_BARS, and its exact identities
with evx_qmix_loss."""
import ctypes as C

import pytest
import torch

import learn_util as lu
from test_qgroup_gpu import GUARD, MIX_BARS, _mixer_errors, _mixer_inputs, _need_gpu

pytestmark = pytest.mark.gpu

GAMMA = 0.99
CASES = [(1, 1, 1), (2, 257, 5), (5, 700, 5), (16, 257, 5)]
MODES = ["sel", "huber", "gamma_row", "all"]


def _options(c, mode, seed):
    """The option inputs of a case: sel [n][B] random actions, gamma_row [B] in (0.5, 1)."""
    g = torch.Generator().manual_seed(seed)
    sel = torch.randint(0, c.A, (c.n, c.B), generator=g, dtype=torch.int32).cuda()
    grow = (0.5 + 0.5 * torch.rand(c.B, generator=g)).cuda()
    return (sel if mode in ("sel", "all") else None), (grow if mode in ("gamma_row", "all") else None)


def _reference(c, dtype, sel=None, delta=0.0, gamma_row=None):
    """_mixer_reference's formula with the options: (loss, mixer gradient flat in state_dict order, dQ
    [n][B][A] scattered at the taken actions, d = q_tot - y [B], the operands' magnitude per row)."""
    from evacx.qmix import MixingNetwork
    n, B, A = c.n, c.B, c.A

    def net(flat):
        m = MixingNetwork(n).to("cuda", dtype)
        m.load_state_dict({k: v.to(dtype) for k, v in lu.mixer_dict(flat, n).items()})
        return m
    mix, mix_t = net(c.mix), net(c.mix_t)
    ai = c.act.long().unsqueeze(2)
    q = c.Q.to(dtype).gather(2, ai).squeeze(2).t().contiguous().requires_grad_(True)  # [B][n]
    Qt = c.Qt.to(dtype)
    with torch.no_grad():
        qt = Qt.max(2)[0] if sel is None else Qt.gather(2, sel.long().clamp(0, A - 1).unsqueeze(2)).squeeze(2)
        gam = GAMMA if gamma_row is None else gamma_row.to(dtype)
        y = c.rew.to(dtype) + gam * mix_t(qt.t()).reshape(B) * (~c.done.bool()).to(dtype)
    d = mix(q).reshape(B) - y.reshape(B)
    if delta > 0:
        ad = d.abs()
        loss = torch.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta)).mean()
    else:
        loss = (d * d).mean()
    loss.backward()
    grad = torch.cat([p.grad.reshape(-1) for p in mix.parameters()])
    dQ = torch.zeros(n, B, A, device="cuda", dtype=dtype)
    dQ.scatter_(2, ai, q.grad.t().unsqueeze(2))
    with torch.no_grad():  # the sum of the magnitudes that enter q_tot and y, per row
        def mag(flat, v):
            sd = lu.mixer_dict(flat, n)
            h = v.abs().double() @ sd["fc1_weight"].abs() + sd["fc1_bias"].abs()
            return (h @ sd["fc2_weight"].abs() + sd["fc2_bias"].abs()).squeeze(-1)
        scale = mag(c.mix, q.detach()) + c.rew.double().abs() + mag(c.mix_t, qt.t())
    return loss.detach(), grad, dQ, d.detach(), scale


def _run(c, sel=None, delta=0.0, gamma_row=None, td=True, opt_null=False, plain=False, nzero=1000):
    """evx_qmix_loss_opt (plain: evx_qmix_loss) on c, every output pre-filled with a sentinel (dQ: 5,
    the rest NaN) and followed by GUARD floats, the zero buffer pre-filled with ones."""
    from evacx._lib import lib
    from evacx.qmlp import td_opts
    L = lib()
    n, B, A = c.n, c.B, c.A
    nm = int(L.evx_qmix_nparams(n))
    npart = int(L.evx_qmix_part_floats(B, n))
    o = lu.SimpleNamespace()
    o.dQ = torch.full((n * B * A + GUARD,), 5.0, device="cuda")
    o.grad = torch.full((nm + GUARD,), float("nan"), device="cuda")
    o.loss = torch.full((1 + GUARD,), float("nan"), device="cuda")
    o.part = torch.full((npart + GUARD,), float("nan"), device="cuda")
    o.td = torch.full((B + GUARD,), float("nan"), device="cuda")
    o.zero = torch.ones(nzero + GUARD, device="cuda")
    args = (c.Q.data_ptr(), c.Qt.data_ptr(), A, c.act.data_ptr(), c.rew.data_ptr(), c.done.data_ptr(), GAMMA, B, n,
            c.mix.data_ptr(), c.mix_t.data_ptr(), o.dQ.data_ptr(), o.grad.data_ptr(), o.loss.data_ptr(),
            o.part.data_ptr(), o.zero.data_ptr(), nzero)
    if plain:
        rc = L.evx_qmix_loss(*args, None)
    else:
        opt = td_opts(sel=sel, huber_delta=delta, gamma_row=gamma_row)
        rc = L.evx_qmix_loss_opt(*args, None if opt_null else C.byref(opt), o.td.data_ptr() if td else None, None)
    torch.cuda.synchronize()
    assert rc == 0, L.evx_qmix_last_error()
    # nothing behind any output, the cleared span exactly
    assert bool((o.dQ[n * B * A:] == 5.0).all()) and bool(torch.isnan(o.grad[nm:]).all())
    assert bool(torch.isnan(o.loss[1:]).all()) and bool(torch.isnan(o.part[npart:]).all())
    assert bool(torch.isnan(o.td[B:]).all()) and (td and not plain or bool(torch.isnan(o.td).all()))
    assert bool((o.zero[nzero:] == 1.0).all()) and torch.count_nonzero(o.zero[:nzero]) == 0
    o.dQ, o.grad, o.loss, o.part, o.td = o.dQ[:n * B * A].view(n, B, A), o.grad[:nm], o.loss[0], o.part[:npart], o.td[:B]
    return o


def _same(a, b, what, names=("loss", "grad", "dQ", "part")):
    for k in names:
        assert torch.equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,B,A", CASES, ids=[f"n{n}-B{b}-A{a}" for n, b, a in CASES])
def test_qmix_opt_kernel_matches_float64(n, B, A, mode):
    """Each option alone and all three together against float64 autograd at MIX_BARS (loss rtol 1e-5;
    mixer gradient rtol 1e-4, atol 1e-5 max |ref|; dQ rtol 1e-4, atol 1e-6 max |ref|), dQ exactly 0 off
    the taken actions over a sentinel, the guards behind every output untouched, two runs bit-equal.

    The Huber delta is the median of the float64 reference's |d|, so the rows split between the two
    branches: at least B // 4 rows on each side (a quarter of the rows; at B = 1 the single row cannot
    lie on both sides, it sits on the boundary |d| = delta, the quadratic branch).

    td_abs against the reference's |d|. The issue's bar is rtol 1e-5. d = tot - y is a difference of two
    f32 values, so where they cancel no f32 evaluation can hold a bar relative to |d|; the test
    therefore splits the rows by the float64 values alone (M = the row's operand magnitude: the sum of
    the absolute values that enter q_tot, y's mixer and the reward):
    * every row: within (2 n + 72) 2^-24 M, the worst case of the f32 evaluation -- each mixer is a dot
      product of n terms plus a bias inside one of 32 terms plus a bias ((n + 34) roundings, each at
      most 2^-24 of the magnitude), then the discount, the reward, the subtraction and the result;
    * rows with |d| >= M / 4: the issue's rtol 1e-5 as it stands (there it allows 42 x 2^-24 M, four
      times the square root of the rounding count). How many rows those are depends on the inputs alone:
      about half with the max target, 5 to 30 % with a random sel (values of either sign enter the
      target mixer and cancel there, against the same M); at least 4 % of the rows must be such rows."""
    _need_gpu()
    c = _mixer_inputs(n, B, A, 100 * n + B + A)
    sel, grow = _options(c, mode, 7 * n + B)
    delta = 0.0
    if mode in ("huber", "all"):
        ad = _reference(c, torch.float64, sel, 0.0, grow)[3].abs()
        delta = float(ad.median().float().item())  # as the kernel gets it: an f32
        lo, hi = int((ad <= delta).sum()), int((ad > delta).sum())
        print(f"huber delta {delta:.6g}: {lo} rows within, {hi} beyond")
        assert lo >= B // 4 and hi >= B // 4 and lo + hi == B
    o = _run(c, sel, delta, grow)
    ref = _reference(c, torch.float64, sel, delta, grow)
    dev = _mixer_errors((o.loss, o.grad, o.dQ), ref[:3])
    f32 = _mixer_errors(_reference(c, torch.float32, sel, delta, grow)[:3], ref[:3])
    ad, td_dev = ref[3].abs(), (o.td.double() - ref[3].abs()).abs()
    td_err = (td_dev / ((2 * n + 72) * 2.0 ** -24 * ref[4])).max().item()  # in units of the worst-case bar
    big = ad >= 0.25 * ref[4]
    td_rel = (td_dev[big] / (1e-5 * ad[big])).max().item()  # in units of the issue's rtol
    print(f"td_abs: {int(big.sum())} of {B} rows with |d| >= M / 4, error / rtol 1e-5 there {td_rel:.3f}")
    assert int(big.sum()) * 25 >= B, "too few rows on which a relative bar means something"
    print(f"n={n} B={B} A={A} {mode}: loss {o.loss.item():.9g} ref {ref[0].item():.9g}; error / bar: kernel " +
          ", ".join(f"{k} {v:.3f}" for k, v in dev.items()) + f", td_abs {td_err:.3f}; float32 torch " +
          ", ".join(f"{k} {v:.3f}" for k, v in f32.items()))
    assert torch.isfinite(o.loss) and torch.isfinite(o.grad).all() and torch.isfinite(o.dQ).all()
    taken = torch.zeros(n, B, A, dtype=torch.bool, device="cuda").scatter_(2, c.act.long().unsqueeze(2), True)
    assert bool((o.dQ[~taken] == 0).all()), "dQ off the taken actions"
    for k, v in dev.items():
        assert v <= 1.0, f"{k} error {v:.3f} x its bar {MIX_BARS[k]} (float32 torch: {f32[k]:.3f})"
    assert td_rel <= 1.0, f"td_abs error {td_rel:.3f} x rtol 1e-5 on the rows with |d| >= M / 4"
    assert td_err <= 1.0, f"td_abs error {td_err:.3f} x the worst-case bar (2 n + 72) 2^-24 M"
    o2 = _run(c, sel, delta, grow)
    _same(o, o2, "two runs", ("loss", "grad", "dQ", "part", "td"))
    o3 = _run(c, sel, delta, grow, td=False)  # td_abs = NULL changes nothing else
    _same(o, o3, "td_abs NULL")


@pytest.mark.parametrize("n,B,A", CASES, ids=[f"n{n}-B{b}-A{a}" for n, b, a in CASES])
def test_qmix_opt_identities_with_the_plain_kernel(n, B, A):
    """Bit for bit against evx_qmix_loss (loss, mixer gradient, dQ and the partial sums): opt = NULL
    (with and without td_abs); an opt with everything off; gamma_row filled with gamma; sel = the index
    of the maximum of Qt; sel outside [0, A) = sel clamped. The Huber loss with delta = 1e30 (no row
    beyond it) gives exactly half the squared-error loss, dQ and mixer gradient: 0.5 (d d) and d / B
    against d d and 2 d / B, every term scaled by a power of two."""
    _need_gpu()
    c = _mixer_inputs(n, B, A, 200 * n + B + A)
    base = _run(c, plain=True)
    _same(base, _run(c, opt_null=True, td=False), "opt NULL, td_abs NULL")
    with_td = _run(c, opt_null=True)
    _same(base, with_td, "opt NULL")
    _same(base, _run(c), "options off")
    _same(base, _run(c, gamma_row=torch.full((B,), GAMMA, device="cuda")), "gamma_row = gamma")
    top = c.Qt.max(2, keepdim=True)[0]
    assert bool(((c.Qt == top).sum(2) == 1).all()), "a tied maximum in the inputs"
    first = c.Qt.argmax(2).to(torch.int32)
    by_sel = _run(c, sel=first)
    _same(base, by_sel, "sel = argmax Qt")
    assert torch.equal(by_sel.td, with_td.td)
    g = torch.Generator().manual_seed(5)
    sel = torch.randint(0, A, (n, B), generator=g, dtype=torch.int32).cuda()
    wild = torch.where(sel == 0, torch.full_like(sel, -3), sel)
    wild = torch.where(sel == A - 1, torch.full_like(sel, A + 7), wild)
    _same(_run(c, sel=sel), _run(c, sel=wild), "sel clamped", ("loss", "grad", "dQ", "part", "td"))
    half = _run(c, delta=1e30)
    assert torch.equal(half.loss * 2, base.loss) and torch.equal(half.dQ * 2, base.dQ)
    assert torch.equal(half.grad * 2, base.grad) and torch.equal(half.td, with_td.td)


def test_qmix_opt_nothing_to_do():
    """B = 0: returns 0 and writes nothing, whatever the options."""
    _need_gpu()
    from evacx._lib import lib
    from evacx.qmlp import td_opts
    c = _mixer_inputs(2, 4, 5, 9)
    nm = 2 * 32 + 65
    dQ = torch.full((64,), 5.0, device="cuda")
    out = torch.full((nm + 1 + 64 + 8,), float("nan"), device="cuda")
    zero = torch.ones(64, device="cuda")
    opt = td_opts(huber_delta=1.0)
    rc = lib().evx_qmix_loss_opt(c.Q.data_ptr(), c.Qt.data_ptr(), 5, c.act.data_ptr(), c.rew.data_ptr(),
                                 c.done.data_ptr(), GAMMA, 0, 2, c.mix.data_ptr(), c.mix_t.data_ptr(), dQ.data_ptr(),
                                 out.data_ptr(), out[nm:].data_ptr(), out[nm + 1:].data_ptr(), zero.data_ptr(), 64,
                                 C.byref(opt), out[nm + 65:].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((dQ == 5.0).all()) and bool(torch.isnan(out).all()) and bool((zero == 1.0).all())
