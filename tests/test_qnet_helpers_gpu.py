"""Every small kernel of the dense learner (csrc/qnet.hip) alone against the plain references of
tests/qnet_helper_util.py (themselves checked in tests/test_qnet_helpers_cpu.py): the kernels
that move data bit for bit, the summing ones against float64 within derived bounds. Every
output lies between two bands of 256 sentinel elements that must come back untouched.

Bounds (u = 2^-24):
  col2im      9 u fold(|dcols|) per element: at most 9 terms are summed.
  sumsq_norm  (T + ceil(parts / 256) + 20) u relative, T = ceil(n / (256 parts)) squares per thread
              (all terms >= 0, so the bound is relative to the result).
  colsum      test_colsum_chunked_tree's bar, 1e-5 max(1, max column sum of |X|); accum adds one
              rounding of |out0| + |sum|.
  clip_adam   K u scale per element with K = 16: twice the K = 8 (measured 7.2) by which the float32
              op-for-op restatement of the kernel stays within the float64 reference on these very
              inputs, on the CPU (test_adam_f32_restatement_meets_K); doubled since the device's
              divide and sqrt may round the last bit the other way. The scales are
              qnet_helper_util.adam_scales'.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import qnet_helper_util as hu
from oracle import oracle as orc
from qnet_helper_util import U, guarded, guards_intact

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _call(name, *args):
    from evacx import _lib, qnet
    _lib.check(getattr(_lib.lib(), name)(*args, qnet._stream()), name)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ exact kernels
@pytest.mark.parametrize("nhwc", [0, 1])
@pytest.mark.parametrize("B,C", [(1, 1), (3, 6), (2, 5), (1, 32), (4, 64)])
def test_im2col_equals_unfold(B, C, nhwc):
    """(4, 64): B*121*C*9 is a multiple of 256 (no ragged last block)."""
    _need_gpu()
    g = torch.Generator().manual_seed(B * 100 + C)
    x = torch.randn(B, C, 11, 11, generator=g)
    src = (x.permute(0, 2, 3, 1) if nhwc else x).contiguous().cuda()
    full, cols = guarded(B * 121 * C * 9)
    _call("evx_im2col3x3", src.data_ptr(), B, C, nhwc, cols.data_ptr())
    torch.cuda.synchronize()
    ref = hu.unfold_ref(x).float()
    assert torch.equal(_bits(cols.cpu().view(B * 121, C * 9)), _bits(ref))
    assert guards_intact(full)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 6, 32, 128, 134, 135, 200])
def test_pix_nchw_both_directions(B, C):
    """C = 134 is the largest LDS tile (65 340 B of dynamic LDS); 135 and 200 take the element-wise
    kernel. Both directions equal the permutation, and the round trip is the identity."""
    _need_gpu()
    g = torch.Generator().manual_seed(B * 1000 + C)
    n = B * 121 * C
    pix = torch.randn(B * 121, C, generator=g)
    nchw = torch.randn(B, C, 121, generator=g)
    pixd, nchwd = pix.cuda(), nchw.cuda()
    f1, d1 = guarded(n)
    _call("evx_pix_nchw", pixd.data_ptr(), B, C, 1, d1.data_ptr())
    f2, d2 = guarded(n)
    _call("evx_pix_nchw", nchwd.data_ptr(), B, C, 0, d2.data_ptr())
    f3, d3 = guarded(n)
    _call("evx_pix_nchw", d1.data_ptr(), B, C, 0, d3.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(d1.cpu().view(B, C, 121)), _bits(hu.pix_to_nchw_ref(pix, B, C)))
    assert torch.equal(_bits(d2.cpu().view(B * 121, C)), _bits(hu.nchw_to_pix_ref(nchw, B, C)))
    assert torch.equal(_bits(d3.cpu().view(B * 121, C)), _bits(pix))
    assert guards_intact(f1) and guards_intact(f2) and guards_intact(f3)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("C", [1, 128, 134])
def test_pix_split_planes_are_bit_equal(B, C):
    """Inputs: +-0, exact bf16 values, ties of the bf16 rounding, 2^-100 .. 2^100."""
    _need_gpu()
    x = hu.split_inputs(B, C, B * 1000 + C)
    n = B * 121 * C
    full, dst = guarded(2 * n, torch.int16)
    xd = x.cuda()
    _call("evx_pix_split", xd.data_ptr(), B, C, dst.data_ptr())
    torch.cuda.synchronize()
    ref = hu.pix_split_ref(x, B, C).reshape(2, n)
    got = dst.cpu().view(2, n)
    assert torch.equal(got[0], ref[0]), "hi plane"
    assert torch.equal(got[1], ref[1]), "lo plane"
    assert guards_intact(full)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_relu_grad_gates_on_y_greater_than_zero(n):
    """y holds +0, -0, 2^-126, negatives and NaN: !(y > 0) zeroes dy, a NaN included."""
    _need_gpu()
    dy, y = hu.relu_inputs(n, n)
    full, d = guarded(n)
    d.copy_(dy)
    yd = y.cuda()
    _call("evx_relu_grad", d.data_ptr(), yd.data_ptr(), n)
    torch.cuda.synchronize()
    ref = hu.relu_grad_ref(dy, y)
    if n > 11:
        assert (ref == 0).any() and (ref != 0).any() and torch.isnan(y).any()
    assert torch.equal(_bits(d.cpu()), _bits(ref))
    assert guards_intact(full)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gather_obs_rows(n):
    """A source of 70 000 rows (indices past 65 535), random, repeated and reversed indices."""
    _need_gpu()
    rows = 70000
    g = torch.Generator().manual_seed(n)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, 8), generator=g, dtype=torch.int64).to(torch.int32)
    srcd = src.cuda()
    rnd = torch.randint(0, rows, (n,), generator=g)
    rnd[0] = rows - 1
    rnd[n // 2] = 65536
    patterns = {"random": rnd, "repeated": torch.full((n,), 65539, dtype=torch.int64),
                "reversed": torch.arange(rows - 1, rows - 1 - n, -1)}
    for name, idx in patterns.items():
        full, dst = guarded(n * 8, torch.int32)
        idxd = idx.cuda()
        _call("evx_gather_obs", srcd.data_ptr(), idxd.data_ptr(), n, dst.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu().view(n, 8), hu.gather_ref(src, idx)), name
        assert guards_intact(full), name


@pytest.mark.parametrize("p", [0.0, 0.2, 1.0])
def test_dropout_mask_equals_the_oracle(p):
    """Element i is lane i % 4 of Philox counter i / 4 + offset under the key 0x5eed."""
    _need_gpu()
    seed = (3 << 32) | 11
    for n in (1, 3, 4, 5, 1023, 4098, 37 * 512):
        for offset in (0, 12345, 2 ** 40 + 7):
            full, m = guarded(n, torch.uint8)
            _call("evx_dropout_mask", m.data_ptr(), n, p, seed, offset)
            torch.cuda.synchronize()
            ref = orc.dropout_mask(n, p, seed, offset)
            assert np.array_equal(m.cpu().numpy(), ref), (n, offset)
            assert guards_intact(full), (n, offset)
    if p == 0.2:  # the offset and the seed matter
        assert not np.array_equal(orc.dropout_mask(4098, p, seed, 0), orc.dropout_mask(4098, p, seed, 12345))


def test_learner_dropout_masks_do_not_reuse_counters():
    """Two successive Learner.dropout_mask(37) calls: the oracle's masks at offsets 0 and
    (37 * 512 + 3) // 4, the counters the first call used being passed over."""
    _need_gpu()
    from evacx.qnet import DROPOUT_P, Learner
    lr = Learner(kind="mlp", precision="exact", seed=9)
    n = 37 * 512
    m1 = lr.dropout_mask(37).cpu().numpy().reshape(-1).copy()
    m2 = lr.dropout_mask(37).cpu().numpy().reshape(-1).copy()
    assert np.array_equal(m1, orc.dropout_mask(n, DROPOUT_P, 9, 0))
    assert np.array_equal(m2, orc.dropout_mask(n, DROPOUT_P, 9, (n + 3) // 4))
    assert not np.array_equal(m1, m2)
    assert lr.rng_offset == 2 * ((n + 3) // 4)


@pytest.mark.parametrize("tau", [0.0, 0.005, 1.0])
@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 3])
def test_polyak_is_bit_equal_to_the_f32_restatement(n, tau):
    """n = 4096 * 256 + 3: three elements past one grid pass."""
    _need_gpu()
    from evacx.qmlp import polyak_coeffs
    r = np.random.RandomState(n % 1000 + int(tau * 1000))
    p = (r.randn(n) * 10.0 ** r.uniform(-6, 2, n)).astype(np.float32)
    t0 = (r.randn(n) * 10.0 ** r.uniform(-6, 2, n)).astype(np.float32)
    t, omt = polyak_coeffs(tau)
    full, td = guarded(n)
    td.copy_(torch.from_numpy(t0))
    pd = torch.from_numpy(p).cuda()
    _call("evx_polyak", pd.data_ptr(), td.data_ptr(), n, t, omt)
    torch.cuda.synchronize()
    ref = hu.polyak_ref_f32(p, t0, t, omt)
    assert np.array_equal(td.cpu().numpy().view(np.int32), ref.view(np.int32))
    assert guards_intact(full)


# ------------------------------------------------------------------ summing kernels
@pytest.mark.parametrize("B,C", [(1, 1), (3, 6), (1, 32), (4, 64)])
def test_col2im_against_fold_in_float64(B, C):
    _need_gpu()
    g = torch.Generator().manual_seed(B * 100 + C)
    dcols = torch.randn(B * 121, C * 9, generator=g)
    dd = dcols.cuda()
    outs = []
    for _ in range(2):
        full, dx = guarded(B * C * 121)
        _call("evx_col2im3x3", dd.data_ptr(), B, C, dx.data_ptr())
        torch.cuda.synchronize()
        assert guards_intact(full)
        outs.append(dx.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    ref = hu.fold_ref(dcols, B, C).reshape(-1)
    bound = 9 * U * hu.fold_ref(dcols.abs(), B, C).reshape(-1)
    err = (outs[0].double() - ref).abs()
    print("col2im worst err / bound", (err / bound).max().item())
    assert (err <= bound).all(), (err / bound).max().item()


@pytest.mark.parametrize("n,scratch_elems", [(1, 2048), (4096, 2048), (4097, 2048), (300000, 1), (300000, 3),
                                             (2048 * 4096 + 5, 2048), (2048 * 4096 + 5, 4096)])
def test_sumsq_norm_against_float64(n, scratch_elems):
    _need_gpu()
    g = torch.Generator().manual_seed(n % 977 + scratch_elems)
    x = torch.randn(n, generator=g)
    fs, scratch = guarded(scratch_elems)
    fn, norm = guarded(1)
    xd = x.cuda()
    _call("evx_sumsq_norm", xd.data_ptr(), n, scratch.data_ptr(), scratch_elems, norm.data_ptr())
    torch.cuda.synchronize()
    ref = hu.norm_ref(x)
    rel = abs(float(norm.item()) - ref) / ref
    print("sumsq rel err / bound", rel / hu.sumsq_bound(n, scratch_elems), "parts", hu.sumsq_parts(n, scratch_elems))
    assert rel <= hu.sumsq_bound(n, scratch_elems), (rel, hu.sumsq_bound(n, scratch_elems))
    assert guards_intact(fs) and guards_intact(fn)


def test_sumsq_norm_of_nothing_is_zero():
    _need_gpu()
    x = torch.ones(4, device="cuda")
    fs, scratch = guarded(8)
    fn, norm = guarded(1)
    _call("evx_sumsq_norm", x.data_ptr(), 0, scratch.data_ptr(), 8, norm.data_ptr())
    torch.cuda.synchronize()
    assert norm.item() == 0.0
    assert guards_intact(fs) and guards_intact(fn)


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("M,N,scratch_elems", [(1000, 37, 16 * 37), (1000, 37, 3 * 37), (1000, 37, 37),
                                               (121, 32, 2 * 32), (1, 5, 5)])
def test_colsum_accum_ld_and_short_scratch(M, N, scratch_elems, pad, accum):
    """accum = 1 adds onto a pre-filled out; ld = N + 7 with the 7 unread columns NaN; the scratch
    starts as NaN, and a scratch below one partial per 64 rows forces chunks = scratch_elems / N
    (16 -> 3 -> 1 chunks at M = 1000)."""
    _need_gpu()
    g = torch.Generator().manual_seed(M + N + scratch_elems)
    ld = N + pad
    X = torch.full((M, ld), float("nan"))
    X[:, :N] = torch.rand(M, N, generator=g) - 0.5
    out0 = torch.randn(N, generator=g) * 3
    fo, out = guarded(N)
    if accum:
        out.copy_(out0)
    fs, scratch = guarded(scratch_elems)
    scratch.fill_(float("nan"))
    Xd = X.cuda()
    _call("evx_colsum", Xd.data_ptr(), ld, M, N, out.data_ptr(), accum, scratch.data_ptr(), scratch_elems)
    torch.cuda.synchronize()
    s = hu.colsum_ref(X, N)
    ref = hu.colsum_ref(X, N, out0 if accum else None)
    bar = 1e-5 * max(1.0, X[:, :N].abs().sum(0).max().item())
    bound = bar + (U * (out0.double().abs() + s.abs()) if accum else 0.0)
    err = (out.cpu().double() - ref).abs()
    assert not torch.isnan(out).any()
    assert (err <= bound).all(), (err.max().item(), bar)
    assert guards_intact(fo) and guards_intact(fs)


@pytest.mark.parametrize("n", list(hu.ADAM_SMALL + hu.ADAM_LARGE))
def test_clip_adam_against_float64(n):
    """K = 16 (see the module docstring). The small sizes cross norm NULL / max_norm 0 / norm below
    / norm above max_norm with weight_decay 0 and 0.01, steps 1, 2, 1000 and betas (0.9, 0.999),
    (0.8, 0.99); the large ones pass one and two grid passes of 4096 x 256 elements. A
    coefficient of 1 without weight decay must hand g back bit-unchanged."""
    _need_gpu()
    from evacx._lib import evx_adam
    worst, ncases = 0.0, 0
    for c in hu.adam_cases(sizes={n}):
        h = c["h"]
        bufs = []
        for a in (c["p"], c["g"], c["m"], c["v"]):
            full, view = guarded(n)
            view.copy_(torch.from_numpy(a))
            bufs.append((full, view))
        norm = None if c["norm"] is None else torch.tensor([float(c["norm"])], dtype=torch.float32, device="cuda")
        hh = evx_adam(lr=float(h.lr), beta1=float(h.beta1), beta2=float(h.beta2), eps=float(h.eps),
                      weight_decay=float(h.weight_decay), step=h.step)
        _call("evx_clip_adam", *(v.data_ptr() for _, v in bufs), n, None if norm is None else norm.data_ptr(),
              float(c["max_norm"]), C.byref(hh))
        torch.cuda.synchronize()
        got = [v.cpu().numpy() for _, v in bufs]
        tag = (c["mode"], float(h.weight_decay), h.step, float(h.beta1))
        assert all(guards_intact(f) for f, _ in bufs), tag
        ref, gc = hu.adam_ref_f64(c["p"], c["g"], c["m"], c["v"], c["norm"], c["max_norm"], h)
        k = hu.adam_units(got, c["p"], gc, ref, h)
        worst, ncases = max(worst, k), ncases + 1
        assert k <= hu.ADAM_K_GPU, (tag, k)
        if not hu.adam_clips(c) and h.weight_decay == 0:
            assert np.array_equal(got[1].view(np.int32), c["g"].view(np.int32)), tag
    print("clip_adam n", n, "cases", ncases, "worst K", worst)
    assert ncases == (48 if n in hu.ADAM_SMALL else 4)
