"""Every kernel route of evx_gemm and evx_conv3x3_gemm on its own, bit-exact against float64.

The cases (gemm_route_cases.py) each name the kernel they reach; before a case launches, its
descriptor's plan (evx_gemm_plan_query, the function gemm_launch switches on) is asserted to be that
route, slice count and reduction. test_gemm_routes_cpu.py holds the same on fake pointers.

Exact data: inputs for which every product and every partial sum is exactly representable in f32,
so the result is the same in any summation order, any K split and all three precisions, and must
equal the float64 reference bit for bit (torch.equal, every element):
  class I  -- A, B integers in [-3, 3]; bias, C0 (ACCUM) and gate integers (9 K < 2^24);
  class H  -- one operand h + m 2^-10 (h in {-1, 0, 1}, m in {-3..3}: its bf16 hi and lo are both
              non-zero wherever h != 0, and hi + lo is the value), the other integers in
              {-1, 0, 1}: every partial sum is a multiple of 2^-10 below 2^14 (K <= 16000). Once
              with the lo part on A ("HA"), once on B ("HB"). A kernel that drops the lo plane is
              off by 2^-10 .. 0.4 per output. For bf16 precision the reference is float64 of the
              bf16-rounded inputs.
alpha (-0.5) and mask_scale (2) are powers of two, so the epilogue is exact too. Every reference
is checked to be exactly representable in f32 before it is compared.

Every C lies in a buffer of the sentinel with guard rows before and after it and, where the case
has ldc > N, padding columns; all of them must still hold the sentinel afterwards. Operand padding
(row strides beyond the row, the float before an offset base) holds NaN.

The rounding pass (randn data, one small shape per route) guards precision only:
  f32   |err| <= (K + 3) 2^-24 bound         (the worst case of any f32 summation order)
  bf16  |err| <= (2^-8 + (K + 3) 2^-24) bound (two operand roundings of 2^-9)
  x3    |err| <= 4e-5 bound + 1e-7            (test_x3_static_table_vs_float64's bar)
  conv  rtol 1e-4, atol 2e-5 max|ref|         (test_conv3x3_implicit_gemm_vs_torch's bar)
with bound = |alpha| (|A| @ |B|) + |bias| (+ |C0|) in float64."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from gemm_route_cases import CONV_CASES, GEMM_CASES, check_plan, conv_args, conv_dims, gemm_args, gemm_strides, gemm_ws

pytestmark = pytest.mark.gpu

SENT = 12345.0      # f32 outputs' sentinel
SENT16 = 0x5A5A     # OUT_SPLIT planes' sentinel (int16)
G = 3               # guard rows before and after C
EXACT = ("I", "HA", "HB")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _gen(name, cls):
    return torch.Generator().manual_seed(zlib.crc32(f"{name}/{cls}".encode()))


def _ints(g, shape, r):
    return torch.randint(-r, r + 1, shape, generator=g).float()


def _class_h(g, shape):
    return _ints(g, shape, 1) + _ints(g, shape, 3) / 1024.0  # exact in f32


def _operands(g, cls, sa, sb, rscale=1.0):
    """The two operands of a data class (shapes sa, sb)."""
    if cls == "I":
        return _ints(g, sa, 3), _ints(g, sb, 3)
    if cls == "HA":
        return _class_h(g, sa), _ints(g, sb, 1)
    if cls == "HB":
        return _ints(g, sa, 1), _class_h(g, sb)
    return torch.randn(sa, generator=g), torch.randn(sb, generator=g) * rscale


def _side(g, cls, shape):
    """bias / C0 / gate values: integers in the exact classes."""
    return _ints(g, shape, 3) if cls != "R" else torch.randn(shape, generator=g)


def _strided(logical, rs, cs, off=0):
    """logical[i][j] at element off + i rs + j cs of a NaN-filled device buffer; (buffer, view at off)."""
    R, Cn = logical.shape
    buf = torch.full((off + (R - 1) * rs + (Cn - 1) * cs + 1,), float("nan"))
    buf[off:].as_strided((R, Cn), (rs, cs)).copy_(logical)
    dev = buf.cuda()
    return dev, dev[off:]


def _planes(x):
    """bf16 hi / lo planes [2][rows][K] of a k-contiguous operand (EVX_GEMM_SPLIT_AB)."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).view(torch.int16).contiguous().cuda()


def _padded(t, ld, fill):
    """t [M][N] as rows of pitch ld on the device."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out.cuda()


def _guards_intact(buf, rows, cols, sent):
    """Everything of buf outside [G, G + rows) x [0, cols) still holds the sentinel."""
    rest = buf.clone()
    rest[G:G + rows, :cols] = sent
    return bool((rest == sent).all())


# ------------------------------------------------------------------ evx_gemm
def run_gemm(c, cls):
    """One pass of a GEMM case on data class cls: (C as computed [M][N], float64 reference, float64
    bound of the rounding bars, the whole C buffer)."""
    from evacx import qnet
    M, N, K, o = c.M, c.N, c.K, c.opts
    g = _gen(c.name, cls)
    A, B = _operands(g, cls, (M, K), (K, N))
    bias = _side(g, cls, (N,)) if "b" in c.epi else None
    C0 = _side(g, cls, (M, N)) if "a" in c.epi else None
    gate = _side(g, cls, (M, N)) if "g" in c.epi else None
    mask = (torch.rand(M, N, generator=g) < 0.75).to(torch.uint8) if "m" in c.epi else None
    mask_scale = 2.0 if cls != "R" else 1.0  # the bars' bound has no mask scale
    alpha = o.get("alpha", 1.0)
    ldc = N + o.get("ldc_pad", 0)
    sam, sak, sbk, sbn = gemm_strides(c)
    if o.get("split_ab"):
        keep, Ad, Bd = None, _planes(A), _planes(B.t().contiguous())
    else:
        ka, Ad = _strided(A, sam, sak, o.get("a_off", 0))
        kb, Bd = _strided(B, sbk, sbn)
        keep = (ka, kb)
    Cbuf = torch.full((G + M + G, ldc), SENT)
    if C0 is not None:
        Cbuf[G:G + M, :N] = C0
    Cbuf = Cbuf.cuda()
    args = gemm_args(c, Ad, Bd, Cbuf[G:], bias=None if bias is None else bias.cuda(),
                     mask=None if mask is None else _padded(mask, N + 3, 0),
                     gate=None if gate is None else _padded(gate, N + 5, 1.0), ws=gemm_ws(c, "cuda"),
                     mask_scale=mask_scale)
    check_plan(c, qnet.gemm_plan(qnet.gemm_desc(**args)))  # with the real pointers and workspace
    qnet.gemm(**args)
    torch.cuda.synchronize()
    out = Cbuf.cpu()
    del keep
    if c.prec == "bf16" and cls != "R":  # the reference of the bf16-rounded inputs (exact as well)
        A, B = A.to(torch.bfloat16).float(), B.to(torch.bfloat16).float()
    ref = alpha * (A.double() @ B.double())
    bound = abs(alpha) * (A.double().abs() @ B.double().abs())
    if bias is not None:
        ref = ref + bias.double()
        bound = bound + bias.double().abs()
    if "r" in c.epi:
        ref = ref.clamp_min(0)
    if mask is not None:
        ref = torch.where(mask.bool(), ref * mask_scale, torch.zeros_like(ref))
    if gate is not None:
        ref = torch.where(gate > 0, ref, torch.zeros_like(ref))
    if C0 is not None:
        ref = ref + C0.double()
        bound = bound + C0.double().abs()
    return out[G:G + M, :N], ref, bound, out


def exact_gemm(c):
    for cls in EXACT:
        got, ref, _, buf = run_gemm(c, cls)
        ref32 = ref.float()
        assert torch.equal(ref32.double(), ref), (c.name, cls, "the reference is not exact in f32")
        if not torch.equal(got, ref32):
            bad = (got != ref32).nonzero()
            i, j = bad[0].tolist()
            raise AssertionError(f"{c.name} [{cls}] route {c.route}: {len(bad)} of {ref.numel()} elements differ, "
                                 f"first C[{i}][{j}] = {got[i, j].item()!r}, reference {ref32[i, j].item()!r}")
        assert _guards_intact(buf, c.M, c.N, SENT), (c.name, cls, "guard rows / padding columns overwritten")


def _family(*prefixes):
    cs = [c for c in GEMM_CASES if c.name.startswith(prefixes)]
    assert cs
    return pytest.mark.parametrize("c", cs, ids=lambda c: c.name)


@_family("f32_")
def test_gemm128_f32_exact(c):
    """gemm128_kernel<float>: four operand layouts, padded strides, neither A stride 1, K 1..100."""
    _need_gpu()
    exact_gemm(c)


@_family("bf16_")
def test_gemm128_bf16_exact(c):
    """gemm128_kernel<__bf16>: the same, and split-K into both reductions (2 slices; 8 slices on
    splitk_reduce4_kernel; 8 slices on splitk_reduce_kernel's non-vector tail)."""
    _need_gpu()
    exact_gemm(c)


@_family("x3_vab_", "x3_va_", "x3_vb_")
def test_gemm128x3_vector_staging_exact(c):
    """gemm128x3_kernel's VA_K | VB_K, VA_K-only and VB_K-only staging."""
    _need_gpu()
    exact_gemm(c)


@_family("x3_sc_")
def test_gemm128x3_scalar_staging_exact(c):
    """gemm128x3_kernel's one-element staging: K % 4 != 0 in each layout, an unaligned A base, a row
    stride that is no multiple of 4, k-major operands kept off tn3_kernel."""
    _need_gpu()
    exact_gemm(c)


@_family("tn3_km_")
def test_tn3_kmajor_exact(c):
    """tn3_kernel<false>: A[k][m], B[k][n]; one pass with each epilogue, and split into slices of 256
    and of 288 rows (not a multiple of the kernel's 64-row chunk)."""
    _need_gpu()
    exact_gemm(c)


@_family("tn3_ak_")
def test_tn3_a_k_contiguous_exact(c):
    """tn3_kernel<false, true>: A[m][k], B[k][n], mask + gate + ACCUM in one pass, and split-K."""
    _need_gpu()
    exact_gemm(c)


@_family("split_ab_")
def test_gemm128x3_split_ab_exact(c):
    """gemm128x3_kernel's SPLIT_AB form on bf16 hi / lo planes: K 8 and 264, ragged M and N, and 8
    slices with the whole epilogue through splitk_reduce4_kernel."""
    _need_gpu()
    exact_gemm(c)


@_family("split_epi_", "ws_cap_")
def test_split_k_epilogue_and_workspace_cap_exact(c):
    """bias + ReLU + mask + gate + ACCUM through splitk_reduce_kernel (4 slices) and
    splitk_reduce4_kernel (8 slices); a workspace of 3 M N floats caps the split at 3 slices of 704,
    one of M N runs a single pass."""
    _need_gpu()
    exact_gemm(c)


def _one_per_route(cases, small):
    seen, out = set(), []
    for c in cases:
        if c.route not in seen and small(c):
            seen.add(c.route)
            out.append(c)
    return out


ROUNDING_GEMM = _one_per_route(GEMM_CASES, lambda c: c.K <= 726 and c.slices == 1 and c.K >= 32) + \
    [c for c in GEMM_CASES if c.name == "bf16_split2"]


@pytest.mark.parametrize("c", ROUNDING_GEMM, ids=lambda c: c.name)
def test_gemm_rounding_pass(c):
    """randn operands through each route once: the error against float64 within the precision's bar."""
    _need_gpu()
    got, ref, bound, buf = run_gemm(c, "R")
    err = (got.double() - ref).abs()
    if c.prec == "f32":
        bar = (c.K + 3) * 2.0 ** -24 * bound
    elif c.prec == "bf16":
        bar = (2.0 ** -8 + (c.K + 3) * 2.0 ** -24) * bound
    else:
        bar = 4e-5 * bound + 1e-7
    print(f"{c.name}: route {c.route}, max err / bound {float((err / (bound + 1e-30)).max()):.3e}")
    assert torch.isfinite(got).all()
    assert (err <= bar).all(), (c.name, float((err / (bound + 1e-30)).max()))
    assert _guards_intact(buf, c.M, c.N, SENT)


def test_rounding_pass_covers_every_gemm_route():
    assert {c.route for c in ROUNDING_GEMM} == {c.route for c in GEMM_CASES}


# ------------------------------------------------------------------ evx_conv3x3_gemm
def nchw(t):
    return t.double().permute(0, 3, 1, 2)


def run_conv(c, cls):
    """One pass of a conv case on data class cls: (output as computed, float64 reference, buffer).
    The lo part ("HA" / "HB") lies on the descriptor's A / B operand: forward X / W, dX dY / W,
    dW dY / X."""
    from evacx import qnet
    cin, cout, Bn = c.cin, c.cout, c.B
    mode, M, N, K, cs = conv_dims(c)
    g = _gen(c.name, cls)
    wsh, xsh, ysh = (cout, cin, 3, 3), (Bn, 11, 11, cin), (Bn, 11, 11, cout)
    x = w = dy = None
    if c.mode == "fwd":
        x, w = _operands(g, cls, xsh, wsh, 0.2)
    elif c.mode == "dx":
        dy, w = _operands(g, cls, ysh, wsh, 0.2)
    else:
        dy, x = _operands(g, cls, ysh, xsh)
    bias = _side(g, cls, (cout,)) if c.mode == "fwd" else None
    below = _side(g, cls, xsh) if c.opts.get("gate") else None
    osp = c.opts.get("out_split", False)
    if osp:
        Cbuf = torch.full((G + 2 * M + G, N), SENT16, dtype=torch.int16).cuda()
    else:
        Cbuf = torch.full((G + M + G, N), SENT).cuda()
    dev = {k: None if t is None else t.contiguous().cuda() for k, t in dict(x=x, w=w, dy=dy, bias=bias, below=below).items()}
    A, Bo = {"fwd": ("x", "w"), "dx": ("dy", "w"), "dw": ("dy", "x")}[c.mode]
    ws = qnet._Workspace() if c.opts.get("ws") else None
    args = conv_args(c, dev[A], dev[Bo], Cbuf[G:G + (2 * M if osp else M)], bias=dev["bias"], gate=dev["below"], ws=ws)
    check_plan(c, qnet.gemm_plan(qnet.conv_desc(**args), mode, cs))
    qnet.conv_gemm(**args)
    torch.cuda.synchronize()
    out = Cbuf.cpu()
    if c.mode == "fwd":
        ref = F.relu(F.conv2d(nchw(x), w.double(), bias.double(), padding=1)).permute(0, 2, 3, 1).reshape(M, N)
    elif c.mode == "dx":
        ref = F.conv_transpose2d(nchw(dy), w.double(), padding=1).permute(0, 2, 3, 1)
        if below is not None:
            ref = ref * (below > 0)
        ref = ref.reshape(M, N)
    else:
        wr = torch.zeros(wsh, dtype=torch.float64, requires_grad=True)
        (ref,) = torch.autograd.grad(F.conv2d(nchw(x), wr, padding=1), wr, nchw(dy))
        ref = ref.reshape(M, N)
    return out[G:G + (2 * M if osp else M)], ref.contiguous(), out


def exact_conv(c):
    _, M, N, _, _ = conv_dims(c)
    osp = c.opts.get("out_split", False)
    for cls in EXACT:
        got, ref, buf = run_conv(c, cls)
        ref32 = ref.float()
        assert torch.equal(ref32.double(), ref), (c.name, cls, "the reference is not exact in f32")
        if osp:  # the planes are bf16(v) and bf16(v - hi) of the exact v
            hi = ref32.to(torch.bfloat16)
            want = torch.cat([hi, (ref32 - hi.float()).to(torch.bfloat16)]).float()
            got = got.view(torch.bfloat16).float()
            assert (want[M:] != 0).any() or cls == "I", "the lo plane under test is all zero"
        else:
            want = ref32
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            i, j = bad[0].tolist()
            raise AssertionError(f"{c.name} [{cls}] route {c.route}: {len(bad)} of {want.numel()} elements differ, "
                                 f"first [{i}][{j}] = {got[i, j].item()!r}, reference {want[i, j].item()!r}")
        assert _guards_intact(buf, 2 * M if osp else M, N, SENT16 if osp else SENT), (c.name, cls, "guard rows")


def _conv_family(*prefixes):
    cs = [c for c in CONV_CASES if c.name.startswith(prefixes)]
    assert cs
    return pytest.mark.parametrize("c", cs, ids=lambda c: c.name)


@_conv_family("lds16_")
def test_conv_lds16_forward_exact(c):
    """conv3x3_x3_kernel<16, 1>: cin 6 (the float2 staging) and cin 5 (the element staging), 1 and 3 images."""
    _need_gpu()
    exact_conv(c)


@_conv_family("wreg32_")
def test_conv_wreg32_forward_exact(c):
    """conv3x3_wreg_kernel<32, ...>: 1, 7, 9 images (a ragged second round of the 8 slots) and 300
    (more than one round per slot)."""
    _need_gpu()
    exact_conv(c)


@_conv_family("lds64_")
def test_conv_lds64_forward_exact(c):
    """conv3x3_x3_kernel<64, 4>: f32 output, and EVX_GEMM_OUT_SPLIT's bf16 hi / lo planes."""
    _need_gpu()
    exact_conv(c)


@_conv_family("dx64_", "dx128_")
def test_conv_lds_dx_exact(c):
    """conv3x3_x3_kernel<64, 1, dX> and <128, 2, dX> with the ReLU gate of the layer below."""
    _need_gpu()
    exact_conv(c)


@_conv_family("gather_")
def test_conv_gathering_exact(c):
    """gemm128x3_kernel<CV_FWD / CV_DX / CV_DW>: odd channels (5 -> 7), the layer shapes without a
    workspace, and dX without a gate (no epilogue: split over K into the workspace)."""
    _need_gpu()
    exact_conv(c)


@_conv_family("tn3_dw_")
def test_conv_dw_tn3_exact(c):
    """tn3_kernel<true> (the conv weight gradient): one pass (K = 363), 2 slices, 17 slices through
    splitk_reduce4_kernel."""
    _need_gpu()
    exact_conv(c)


ROUNDING_CONV = _one_per_route(CONV_CASES, lambda c: not c.opts.get("out_split") and c.slices == 1)


@pytest.mark.parametrize("c", ROUNDING_CONV, ids=lambda c: c.name)
def test_conv_rounding_pass(c):
    """randn activations and weights through each conv route once, at test_conv3x3_implicit_gemm_vs_torch's bar."""
    _need_gpu()
    _, M, N, _, _ = conv_dims(c)
    got, ref, buf = run_conv(c, "R")
    ref = ref.float()
    print(f"{c.name}: route {c.route}, max err {float((got - ref).abs().max()):.3e}, max |ref| {float(ref.abs().max()):.3e}")
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=2e-5 * ref.abs().max().item())
    assert _guards_intact(buf, M, N, SENT)


def test_rounding_pass_covers_every_conv_route():
    assert {c.route for c in ROUNDING_CONV} == {c.route for c in CONV_CASES}
