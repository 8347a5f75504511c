"""The dense learner's helper kernels without a device: (1) the references of
tests/qnet_helper_util.py held to account -- the Adam restatement against clip_grad_norm_ +
torch.optim.Adam in float64, unfold against fold as adjoints, oracle.dropout_mask against its
own laws and a Python restatement; (2) the measured K of the clip + Adam bound; (3) every
entry's refusals (-22 with a named message) before any launch, with NULL or dummy pointers
that are never dereferenced."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import qnet_helper_util as hu
from oracle import oracle as orc


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", ["above", "below"])
def test_adam_reference_is_torch_adam_in_float64(wd, clip):
    """adam_step64 over steps 1..3 gives the p, exp_avg, exp_avg_sq and clipped grads of
    clip_grad_norm_ + torch.optim.Adam run on CPU float64 tensors (both are float64 runs of the
    same formulas: 1e-12 relative covers the two evaluation orders)."""
    r = np.random.RandomState(3)
    n = 257
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p = r.randn(n) * 0.1
    m, v = np.zeros(n), np.zeros(n)
    param = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([param], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for step in (1, 2, 3):
        g = r.randn(n) * 10.0 ** r.uniform(-6, 0, n)
        gn = math.sqrt(float((g ** 2).sum()))
        max_norm = 0.37 * gn if clip == "above" else 2 * gn + 1
        param.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_([param], max_norm)
        assert abs(total.item() - gn) <= 1e-12 * gn
        g_torch = param.grad.clone().numpy()
        opt.step()
        coef = min(max_norm / (gn + 1e-6), 1.0)
        assert (coef < 1.0) == (clip == "above")
        (pn, _, mn, vn, _), gc = hu.adam_step64(p, g, m, v, coef, b1, b2, eps, wd, lr / (1 - b1 ** step),
                                                math.sqrt(1 - b2 ** step))
        st = opt.state[param]
        np.testing.assert_allclose(gc, g_torch, rtol=1e-12, atol=0)
        if clip == "below":
            assert np.array_equal(gc, g)
        np.testing.assert_allclose(mn, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(vn, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(pn, param.detach().numpy(), rtol=1e-12, atol=0)
        p, m, v = pn, mn, vn


def test_adam_hyper_scalars_are_the_launchers():
    """AdamHyper derives step_size and sqrt(bias correction 2) as evx_clip_adam does: in double from
    the float32 fields, rounded to float32 once."""
    h = hu.AdamHyper(lr=1e-3, beta1=0.9, beta2=0.999, step=2)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert h.step_size == np.float32(float(np.float32(1e-3)) / (1.0 - b1 * b1))
    assert h.bc2_sqrt == np.float32(math.sqrt(1.0 - b2 * b2))
    # 1 - beta is exact in float32 for the betas of the tests (Sterbenz), so the kernel's 1.f - beta
    # and the float64 reference's 1 - beta are the same number
    for b in (0.9, 0.999, 0.8, 0.99):
        assert float(np.float32(1.0) - np.float32(b)) == 1.0 - float(np.float32(b))


def test_adam_f32_restatement_meets_K():
    """The measurement behind the GPU bound: over every input of adam_cases() the float32 op-for-op
    restatement of clip_adam_kernel is within ADAM_K_CPU * 2^-24 * scale of the float64 reference,
    and ADAM_K_CPU is the smallest such integer (measured 7.2 -> 8; the GPU test allows 16)."""
    worst = 0.0
    for c in hu.adam_cases():
        args = (c["p"], c["g"], c["m"], c["v"], c["norm"], c["max_norm"], c["h"])
        ref, gc = hu.adam_ref_f64(*args)
        got = hu.adam_ref_f32(*args)
        worst = max(worst, hu.adam_units(got, c["p"], gc, ref, c["h"]))
        if not hu.adam_clips(c) and c["h"].weight_decay == 0:
            assert np.array_equal(got[1], c["g"])  # coefficient 1: g comes back bit-unchanged
    assert math.ceil(worst) == hu.ADAM_K_CPU, worst
    assert hu.ADAM_K_GPU == 2 * hu.ADAM_K_CPU


def test_adam_cases_cover_the_issue():
    cs = list(hu.adam_cases())
    assert {c["n"] for c in cs} == {1, 255, 257, 4096 * 256 + 3, 2 * 4096 * 256 + 1}
    small = [c for c in cs if c["n"] <= 257]
    assert len(small) == 3 * 4 * 2 * 3 * 2
    for mode in hu.ADAM_NORM_MODES:
        sel = [c for c in cs if c["mode"] == mode]
        assert all(hu.adam_clips(c) == (mode == "above") for c in sel)
        assert {c["n"] for c in sel} == {c["n"] for c in cs}
    g = np.concatenate([c["g"] for c in cs if c["n"] > 1])
    v = np.concatenate([c["v"] for c in cs if c["n"] > 1])
    assert ((g == 0) & (v == 0)).any() and (np.abs(g[g != 0]) <= 1e-12).any()


@pytest.mark.parametrize("B,C", [(1, 1), (3, 6), (2, 5)])
def test_unfold_and_fold_are_adjoint(B, C):
    """<unfold(x), c> == <x, fold(c)> in float64, and unfold's column order is k = c*9 + ky*3 + kx
    of the pixel's 3x3 neighbourhood (zero outside the map)."""
    g = torch.Generator().manual_seed(B * 10 + C)
    x = torch.randn(B, C, 11, 11, generator=g, dtype=torch.float64)
    c = torch.randn(B * 121, C * 9, generator=g, dtype=torch.float64)
    lhs = (hu.unfold_ref(x) * c).sum().item()
    rhs = (x * hu.fold_ref(c, B, C)).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * (hu.unfold_ref(x).abs() * c.abs()).sum().item()
    u = hu.unfold_ref(x)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    for b, ch, y, xx, ky, kx in [(0, 0, 0, 0, 0, 0), (B - 1, C - 1, 10, 10, 2, 2), (B - 1, C // 2, 4, 7, 1, 2),
                                 (0, C - 1, 0, 10, 2, 0)]:
        assert u[b * 121 + y * 11 + xx, ch * 9 + ky * 3 + kx] == xp[b, ch, y + ky, xx + kx]


def test_pix_references_are_inverse_and_split_is_hi_plus_lo():
    B, C = 2, 5
    x = hu.split_inputs(B, C, 1)
    assert torch.equal(hu.pix_to_nchw_ref(hu.nchw_to_pix_ref(x, B, C), B, C), x)
    pl = hu.pix_split_ref(x, B, C).view(torch.bfloat16).float()
    pix = hu.nchw_to_pix_ref(x, B, C).reshape(B, 121 * C)
    # bf16 keeps 8 significant bits: hi is within 2^-8 relative (half an ulp), hi + lo within 2^-16
    assert ((pl[0] - pix).abs() <= 2.0 ** -8 * pix.abs()).all()
    assert ((pl[0].double() + pl[1].double() - pix.double()).abs() <= 2.0 ** -16 * pix.abs().double()).all()
    flat = x.reshape(-1).view(torch.int32)
    k = torch.arange(flat.numel()) % 7
    assert ((flat[k == 2] & 0xFFFF) == 0x8000).all() and ((flat[k == 3] & 0x1FFFF) == 0x18000).all()
    # ties go to the even kept mantissa: down on k == 2, up on k == 3
    hi_bits = hu.nchw_to_pix_ref(x, B, C).reshape(-1).to(torch.bfloat16).view(torch.int16).int() & 0xFFFF
    src_bits = hu.nchw_to_pix_ref(x, B, C).reshape(-1).view(torch.int32)
    kk = hu.nchw_to_pix_ref(k.reshape(B, C, 121).float(), B, C).reshape(-1).long()
    up = (src_bits >> 16) & 0xFFFF
    assert (hi_bits[kk == 2] == up[kk == 2]).all()
    assert (hi_bits[kk == 3] == ((up[kk == 3] + 1) & 0xFFFF)).all()


def test_polyak_restatement_rounds_three_times():
    p = np.array([1.0, 3.0, -0.1], np.float32)
    t = np.array([1.0, 5.0, 0.7], np.float32)
    tau, omt = np.float32(0.005), np.float32(1.0 - float(np.float32(0.005)))
    want = (np.float32(tau * p).astype(np.float32) + np.float32(omt * t)).astype(np.float32)
    got = hu.polyak_ref_f32(p, t, tau, omt)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(hu.polyak_ref_f32(p, t, 0.0, 1.0), t)
    assert np.array_equal(hu.polyak_ref_f32(p, t, 1.0, 0.0), p)


# ------------------------------------------------------------------ oracle.dropout_mask
def _philox_mask(n, p, seed, offset, key2):
    """evx_dropout_mask's rule in Python on the oracle's Philox4x32-10 (itself pinned by the published
    known-answer vectors, tests/test_prio_cpu.py), with the counter's third word given."""
    L = orc.lib()
    out = np.zeros(n, np.uint8)
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    r = (C.c_uint32 * 4)()
    for i4 in range(0, n, 4):
        c = (i4 // 4 + offset) & (2 ** 64 - 1)
        ctr = (C.c_uint32 * 4)(c & 0xFFFFFFFF, c >> 32, key2, 0)
        L.orc_philox4x32_10(ctr, key, r)
        for j in range(min(4, n - i4)):
            u = np.float32(r[j] >> 8) * np.float32(1.0 / 16777216.0)
            out[i4 + j] = 1 if u >= np.float32(p) else 0
    return out


def test_oracle_dropout_mask_laws():
    n = 1 << 20
    for p in (0.2, 0.5):
        rate = orc.dropout_mask(n, p, 11, 0).mean()
        sigma = math.sqrt(p * (1 - p) / n)
        assert abs(rate - (1 - p)) <= 4 * sigma, (p, rate)
    assert orc.dropout_mask(4099, 0.0, 5, 7).all()
    assert not orc.dropout_mask(4099, 1.0, 5, 7).any()
    assert orc.dropout_mask(0, 0.2, 5, 7).size == 0
    # counters advance by one per 4 elements: a mask is its first n1 elements followed by the mask
    # that starts n1 / 4 counters later
    for n1, n2, o in [(4, 5, 0), (1024, 3075, 12345), (37 * 512, 37 * 512, 2 ** 40 + 7), (8, 1, 2 ** 64 - 2)]:
        whole = orc.dropout_mask(n1 + n2, 0.2, 9, o)
        parts = np.concatenate([orc.dropout_mask(n1, 0.2, 9, o), orc.dropout_mask(n2, 0.2, 9, o + n1 // 4)])
        assert np.array_equal(whole, parts), (n1, n2, o)
    # another seed, another offset: another mask
    a = orc.dropout_mask(4096, 0.2, 9, 0)
    assert not np.array_equal(a, orc.dropout_mask(4096, 0.2, 10, 0))
    assert not np.array_equal(a, orc.dropout_mask(4096, 0.2, 9, 1))
    assert np.array_equal(a[4:], orc.dropout_mask(4092, 0.2, 9, 1))


@pytest.mark.parametrize("offset", [0, 12345, 2 ** 40 + 7])
def test_oracle_dropout_mask_is_its_philox_rule(offset):
    """Element i is lane i % 4 of counter (i / 4 + offset, 0x5eed, 0) under the seed's key -- and not
    the act draw's counter (0xac7), whose mask differs."""
    n, p, seed = 4099, 0.2, (7 << 32) | 3
    a = orc.dropout_mask(n, p, seed, offset)
    assert np.array_equal(a, _philox_mask(n, p, seed, offset, 0x5EED))
    act = _philox_mask(n, p, seed, offset, 0xAC7)
    assert not np.array_equal(a, act) and abs((a != act).mean() - 2 * 0.2 * 0.8) < 0.05


# ------------------------------------------------------------------ refusals before any launch
def _L():
    from evacx import _lib
    return _lib.lib()


def _refused(rc, text):
    L = _L()
    err = L.evx_q_last_error()
    assert rc == -22 and text in err, (rc, err)


BUF = (C.c_float * 64)()  # a non-NULL dummy: every call below fails or returns before it is read


def _null_each(call, nptr, text):
    """call(*pointers) with each of its nptr pointers NULL in turn (the others the dummy)."""
    for k in range(nptr):
        ptrs = [None if j == k else BUF for j in range(nptr)]
        _refused(call(*ptrs), text)


def test_null_pointers_are_refused():
    L = _L()
    h = _adam()
    _null_each(lambda X, out, sc: L.evx_colsum(X, 8, 4, 8, out, 0, sc, 64, None), 3, b"colsum: NULL")
    _null_each(lambda g, sc, nrm: L.evx_sumsq_norm(g, 16, sc, 64, nrm, None), 3, b"sumsq: NULL")
    _null_each(lambda p, g, m, v: L.evx_clip_adam(p, g, m, v, 16, BUF, 1.0, C.byref(h), None), 4, b"adam: NULL")
    _refused(L.evx_clip_adam(BUF, BUF, BUF, BUF, 16, BUF, 1.0, None, None), b"adam: NULL")
    _refused(L.evx_dropout_mask(None, 16, 0.2, 1, 0, None), b"dropout_mask: NULL")
    _null_each(lambda s, i, d: L.evx_gather_obs(s, i, 2, d, None), 3, b"gather_obs: NULL")
    _null_each(lambda x, c: L.evx_im2col3x3(x, 1, 1, 0, c, None), 2, b"im2col: NULL")
    _null_each(lambda c, x: L.evx_col2im3x3(c, 1, 1, x, None), 2, b"col2im: NULL")
    _null_each(lambda s, d: L.evx_pix_split(s, 1, 1, d, None), 2, b"pix_split: NULL")
    for to_nchw in (0, 1):
        for ch in (1, 200):  # the LDS kernel and the element-wise one
            _null_each(lambda s, d: L.evx_pix_nchw(s, 1, ch, to_nchw, d, None), 2, b"pix_nchw: NULL")
    _null_each(lambda dy, y: L.evx_relu_grad(dy, y, 4, None), 2, b"relu_grad: NULL")
    _null_each(lambda p, t: L.evx_polyak(p, t, 4, 0.5, 0.5, None), 2, b"polyak: NULL")


def _adam(**kw):
    from evacx._lib import evx_adam
    f = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1)
    f.update(kw)
    return evx_adam(**f)


@pytest.mark.parametrize("field,bad,text", [
    ("step", 0, b"step"), ("step", -3, b"step"),
    ("beta1", 1.0, b"betas"), ("beta1", -0.1, b"betas"), ("beta1", math.nan, b"betas"), ("beta1", 1.5, b"betas"),
    ("beta2", 1.0, b"betas"), ("beta2", -0.1, b"betas"), ("beta2", math.nan, b"betas"), ("beta2", math.inf, b"betas"),
    ("lr", math.inf, b"lr and eps"), ("lr", math.nan, b"lr and eps"),
    ("eps", -math.inf, b"lr and eps"), ("eps", math.nan, b"lr and eps")])
def test_clip_adam_refuses_bad_hyper_parameters(field, bad, text):
    """step = 0 would make 1 - beta^step = 0 and lr / 0 an infinity in every parameter; the refusal
    comes whatever else is passed, a zero-size call included."""
    L = _L()
    h = _adam(**{field: bad})
    for n in (16, 0):
        _refused(L.evx_clip_adam(BUF, BUF, BUF, BUF, n, BUF, 1.0, C.byref(h), None), b"adam: " + text)
    for ok in (_adam(beta1=0.0, beta2=0.0), _adam(step=1000)):  # the edges of the ranges pass
        assert L.evx_clip_adam(BUF, BUF, BUF, BUF, 0, BUF, 1.0, C.byref(ok), None) == 0


def test_sumsq_norm_refuses_an_empty_scratch():
    L = _L()
    for se in (0, -1):
        for n in (16, 0):
            _refused(L.evx_sumsq_norm(BUF, n, BUF, se, BUF, None), b"sumsq: scratch_elems")


@pytest.mark.parametrize("p", [-0.1, 1.5, math.nan, math.inf, -math.inf])
def test_dropout_mask_refuses_p_outside_unit_interval(p):
    L = _L()
    for n in (16, 0):
        _refused(L.evx_dropout_mask(BUF, n, p, 1, 0, None), b"dropout_mask: p")


@pytest.mark.parametrize("ch", [0, -1, -(2 ** 31)])
def test_conv_helpers_refuse_no_channels(ch):
    L = _L()
    for nhwc in (0, 1):
        _refused(L.evx_im2col3x3(BUF, 2, ch, nhwc, BUF, None), b"im2col: C")
        _refused(L.evx_pix_nchw(BUF, 2, ch, nhwc, BUF, None), b"pix_nchw: C")
    _refused(L.evx_col2im3x3(BUF, 2, ch, BUF, None), b"col2im: C")
    _refused(L.evx_pix_split(BUF, 2, ch, BUF, None), b"pix_split: C")


def test_pix_split_still_refuses_more_than_134_channels():
    _refused(_L().evx_pix_split(BUF, 1, 135, BUF, None), b"pix_split: C > 134")


def test_zero_size_calls_return_0():
    """n <= 0 or B <= 0: nothing to do, 0 -- with NULL pointers and any channel count."""
    L = _L()
    h = _adam()
    for z in (0, -5):
        assert L.evx_colsum(None, 8, z, 8, None, 0, None, 0, None) == 0
        assert L.evx_colsum(None, 8, 4, z, None, 0, None, 0, None) == 0
        assert L.evx_clip_adam(None, None, None, None, z, None, 1.0, C.byref(h), None) == 0
        assert L.evx_dropout_mask(None, z, 0.2, 1, 0, None) == 0
        assert L.evx_gather_obs(None, None, z, None, None) == 0
        assert L.evx_relu_grad(None, None, z, None) == 0
        assert L.evx_polyak(BUF, BUF, z, 0.5, 0.5, None) == 0
        for ch in (0, 1, 200):
            assert L.evx_im2col3x3(None, z, ch, 1, None, None) == 0
            assert L.evx_col2im3x3(None, z, ch, None, None) == 0
            assert L.evx_pix_split(None, z, ch, None, None) == 0
            assert L.evx_pix_nchw(None, z, ch, 1, None, None) == 0
