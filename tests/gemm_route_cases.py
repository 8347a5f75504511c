"""The case tables of the GEMM / conv3x3 route tests, shared by test_gemm_routes_cpu.py (every case
plans as intended: evx_gemm_plan_query on fake pointers) and test_gemm_routes_gpu.py (every case
computes the float64 reference bit for bit on the route it names).

A case names the route it is meant to reach (an evacx._lib.ROUTE key), the K slices and the
split-K reduction (an evacx._lib.REDUCE key). Both tests build the descriptor through
evacx.qnet.gemm_desc / conv_desc from the same arguments (gemm_args / conv_args below), so the
descriptor the CPU test plans is the descriptor the GPU test launches.

Epilogues ("" none): b bias, r ReLU, m dropout mask (ldm = N + 3, scale 2), g gate (ldg = N + 5),
a ACCUM; alpha = -0.5 and ldc = N + 7 ride in the options.
Layouts: A "mk" A[m][k] (sak 1) or "km" A[k][m] (sam 1); B "nk" B[n][k] (sbk 1) or "kn" B[k][n] (sbn 1).
Options: pad_a / pad_b (row stride beyond the row's length), a_step (distance between consecutive
elements of A: 2 leaves neither A stride 1), a_off (A's base moved by that many floats: 1 is not
16-byte aligned), alpha, ldc_pad, ws ("pool": the full split's workspace; an integer f: a workspace
of f * M * N floats; None: none), split_ab, klen (the expected slice length)."""
from collections import namedtuple

import torch

GemmCase = namedtuple("GemmCase", "name prec M N K layout epi opts route slices reduce")
ConvCase = namedtuple("ConvCase", "name mode cin cout B opts route slices reduce")

ALL = "brmga"
DAGGER = dict(alpha=-0.5, ldc_pad=7)  # alpha != 1 and ldc > N together


def _g(name, prec, M, N, K, layout, epi, route, slices=1, reduce="NONE", **opts):
    return GemmCase(name, prec, M, N, K, layout, epi, opts, route, slices, reduce)


def _gemm128(prec):
    """gemm128_kernel<float> / <__bf16>: the four layouts, padded strides, neither A stride 1,
    K in {1, 31, 32, 33, 100}; one side of the 128 tile ragged and the other not."""
    r = "GEMM128_F32" if prec == "f32" else "GEMM128_BF16"
    return [
        _g(f"{prec}_mk_nk", prec, 33, 128, 33, "mk nk", "", r),
        _g(f"{prec}_mk_kn", prec, 128, 31, 100, "mk kn", "br", r),
        _g(f"{prec}_km_kn", prec, 129, 128, 31, "km kn", "brm", r),
        _g(f"{prec}_km_nk", prec, 1, 128, 32, "km nk", "g", r),
        _g(f"{prec}_padded", prec, 127, 128, 1, "mk nk", "a", r, pad_a=3, pad_b=5),
        _g(f"{prec}_a_step2", prec, 128, 130, 100, "mk kn", "", r, a_step=2, **DAGGER),
        _g(f"{prec}_km_padded", prec, 132, 128, 33, "km kn", "g", r, pad_a=1, pad_b=2, ldc_pad=7),
    ]


GEMM_CASES = _gemm128("f32") + _gemm128("bf16") + [
    # bf16 split-K (no epilogue: K >= 512 splits into slices of >= 256)
    _g("bf16_split2", "bf16", 36, 20, 512, "mk nk", "", "GEMM128_BF16", 2, "GENERIC", ws="pool"),
    _g("bf16_split8_reduce4", "bf16", 36, 20, 2048, "km kn", "a", "GEMM128_BF16", 8, "QUARTERS", ws="pool"),
    _g("bf16_split8_tail", "bf16", 5, 7, 2048, "mk kn", "", "GEMM128_BF16", 8, "GENERIC", ws="pool", **DAGGER),
    # x3, A and B from 16-B loads
    _g("x3_vab_k4", "x3", 33, 128, 4, "mk nk", "", "X3_VEC_AB"),
    _g("x3_vab_k36", "x3", 128, 31, 36, "mk nk", "brm", "X3_VEC_AB"),
    _g("x3_vab_k260", "x3", 132, 128, 260, "mk nk", "g", "X3_VEC_AB"),
    _g("x3_vab_alpha", "x3", 127, 128, 36, "mk nk", "br", "X3_VEC_AB", **DAGGER),
    _g("x3_vab_accum", "x3", 128, 129, 260, "mk nk", "a", "X3_VEC_AB", pad_a=4, pad_b=8),
    # x3, A only
    _g("x3_va_k100", "x3", 33, 128, 100, "mk kn", "br", "X3_VEC_A"),
    _g("x3_va_k260", "x3", 128, 130, 260, "mk kn", "a", "X3_VEC_A"),
    _g("x3_va_alpha", "x3", 1, 128, 100, "mk kn", "g", "X3_VEC_A", **DAGGER),
    # x3, B only
    _g("x3_vb_k36", "x3", 128, 33, 36, "km nk", "g", "X3_VEC_B"),
    _g("x3_vb_k260", "x3", 31, 128, 260, "km nk", "brm", "X3_VEC_B", **DAGGER),
    _g("x3_vb_a_unaligned", "x3", 128, 130, 36, "mk nk", "", "X3_VEC_B", a_off=1),
    # x3, one element per load: K % 4 != 0 in each layout, an unaligned base, a row stride % 4 != 0,
    # K >= 256 k-major operands off tn3_kernel by alignment
    _g("x3_sc_mk_nk", "x3", 33, 128, 33, "mk nk", "", "X3_SCALAR"),
    _g("x3_sc_mk_kn", "x3", 128, 31, 33, "mk kn", "br", "X3_SCALAR"),
    _g("x3_sc_km_kn", "x3", 129, 128, 33, "km kn", "brm", "X3_SCALAR"),
    _g("x3_sc_km_nk", "x3", 128, 127, 33, "km nk", "a", "X3_SCALAR"),
    _g("x3_sc_a_unaligned", "x3", 130, 128, 36, "mk kn", "g", "X3_SCALAR", a_off=1),
    _g("x3_sc_sam_k1", "x3", 128, 132, 36, "mk kn", "", "X3_SCALAR", pad_a=1, **DAGGER),
    _g("x3_sc_kmajor_unaligned", "x3", 4, 132, 260, "km kn", "br", "X3_SCALAR", a_off=1),
    _g("x3_sc_kmajor_alpha", "x3", 132, 4, 256, "km kn", "", "X3_SCALAR", **DAGGER),
    # tn3_kernel, A k-major
    _g("tn3_km_k256", "x3", 4, 132, 256, "km kn", "", "TN3_KMAJOR"),
    _g("tn3_km_k260", "x3", 132, 4, 260, "km kn", "br", "TN3_KMAJOR"),
    _g("tn3_km_k324", "x3", 132, 132, 324, "km kn", "brm", "TN3_KMAJOR"),
    _g("tn3_km_gate", "x3", 4, 4, 256, "km kn", "g", "TN3_KMAJOR", ldc_pad=7),
    _g("tn3_km_accum", "x3", 132, 4, 324, "km kn", "a", "TN3_KMAJOR", pad_a=4, pad_b=4),
    _g("tn3_km_split256", "x3", 36, 20, 2048, "km kn", "", "TN3_KMAJOR", 8, "QUARTERS", ws="pool", klen=256),
    _g("tn3_km_split288", "x3", 36, 20, 2084, "km kn", "a", "TN3_KMAJOR", 8, "QUARTERS", ws="pool", klen=288,
       ldc_pad=7),
    # tn3_kernel, A k-contiguous
    _g("tn3_ak_k256", "x3", 132, 36, 256, "mk kn", ALL, "TN3_AK"),
    _g("tn3_ak_k1028", "x3", 4, 4, 1028, "mk kn", "mga", "TN3_AK"),
    _g("tn3_ak_gate", "x3", 132, 36, 256, "mk kn", "g", "TN3_AK", pad_a=4, pad_b=4, ldc_pad=7),
    _g("tn3_ak_split", "x3", 36, 20, 2084, "mk kn", "", "TN3_AK", 8, "QUARTERS", ws="pool", klen=288),
    # pre-split planes
    _g("split_ab_k8", "x3", 33, 31, 8, "mk nk", "br", "X3_SPLIT_AB", split_ab=True),
    _g("split_ab_k264", "x3", 129, 127, 264, "mk nk", "", "X3_SPLIT_AB", split_ab=True, **DAGGER),
    _g("split_ab_split8", "x3", 8, 12, 8192, "mk nk", ALL, "X3_SPLIT_AB", 8, "QUARTERS", ws="pool", split_ab=True,
       klen=1024),
    # split-K with the whole epilogue through the reduction
    _g("split_epi_4", "x3", 8, 4, 4096, "mk nk", ALL, "X3_VEC_AB", 4, "GENERIC", ws="pool", klen=1024),
    _g("split_epi_8", "x3", 8, 12, 8192, "mk nk", ALL, "X3_VEC_AB", 8, "QUARTERS", ws="pool", klen=1024, ldc_pad=7),
    # the workspace caps the slice count
    _g("ws_cap_3", "x3", 130, 36, 2048, "mk nk", "", "X3_VEC_AB", 3, "GENERIC", ws=3, klen=704),
    _g("ws_cap_1", "x3", 130, 36, 2048, "mk nk", "", "X3_VEC_AB", 1, "NONE", ws=1),
]


def _c(name, mode, cin, cout, B, route, slices=1, reduce="NONE", **opts):
    return ConvCase(name, mode, cin, cout, B, opts, route, slices, reduce)


# ws=True: a _Workspace (QNet's calls); gate: dX with the ReLU gate of the layer below
CONV_CASES = (
    [_c(f"lds16_c{ci}_b{B}", "fwd", ci, 32, B, "CONV_LDS16_FWD", ws=True) for ci in (6, 5) for B in (1, 3)] +
    [_c(f"wreg32_b{B}", "fwd", 32, 64, B, "CONV_WREG32_FWD", ws=True) for B in (1, 7, 9, 300)] +
    [_c(f"lds64_b{B}", "fwd", 64, 128, B, "CONV_LDS64_FWD", ws=True) for B in (1, 3)] +
    [_c(f"lds64_outsplit_b{B}", "fwd", 64, 128, B, "CONV_LDS64_FWD", ws=True, out_split=True) for B in (1, 3)] +
    [_c(f"dx64_b{B}", "dx", 32, 64, B, "CONV_LDS64_DX", ws=True, gate=True) for B in (1, 3)] +
    [_c(f"dx128_b{B}", "dx", 64, 128, B, "CONV_LDS128_DX", ws=True, gate=True) for B in (1, 3)] +
    [   # the gathering kernels: no workspace, or shapes the staged kernels do not take
        _c("gather_fwd_5_7", "fwd", 5, 7, 4, "X3_CONV_FWD"),
        _c("gather_dx_5_7", "dx", 5, 7, 4, "X3_CONV_DX", gate=True),
        _c("gather_dw_5_7", "dw", 5, 7, 4, "X3_CONV_DW"),
        _c("gather_fwd_conv1", "fwd", 6, 32, 2, "X3_CONV_FWD"),
        _c("gather_fwd_conv2", "fwd", 32, 64, 2, "X3_CONV_FWD"),
        _c("gather_fwd_conv3", "fwd", 64, 128, 2, "X3_CONV_FWD"),
        _c("gather_dx_conv2", "dx", 32, 64, 2, "X3_CONV_DX", gate=True),
        _c("gather_dx_conv3", "dx", 64, 128, 2, "X3_CONV_DX", gate=True),
        _c("gather_dw_conv1", "dw", 6, 32, 2, "X3_CONV_DW"),
        _c("gather_fwd_5_7_ws", "fwd", 5, 7, 4, "X3_CONV_FWD", ws=True),
        # dX without a gate has no epilogue: with a workspace it splits K and leaves the staged kernel
        _c("gather_dx_nogate_split", "dx", 32, 64, 1, "X3_CONV_DX", 2, "GENERIC", ws=True, klen=288),
        # conv dW on tn3_kernel
        _c("tn3_dw_b3", "dw", 32, 64, 3, "TN3_CONV_DW", ws=True),
        _c("tn3_dw_b3_nows", "dw", 32, 64, 3, "TN3_CONV_DW"),
        _c("tn3_dw_b5", "dw", 32, 64, 5, "TN3_CONV_DW", 2, "GENERIC", ws=True, klen=320),
        _c("tn3_dw_b40", "dw", 32, 64, 40, "TN3_CONV_DW", 17, "QUARTERS", ws=True, klen=288),
    ])


# ------------------------------------------------------------------ descriptors
def gemm_strides(c):
    """(sam, sak, sbk, sbn) of a GEMM case."""
    o, (la, lb) = c.opts, c.layout.split()
    step = o.get("a_step", 1)
    if la == "mk":
        sam, sak = (c.K + o.get("pad_a", 0)) * step, step
    else:
        sam, sak = step, (c.M + o.get("pad_a", 0)) * step
    if lb == "nk":
        sbk, sbn = 1, c.K + o.get("pad_b", 0)
    else:
        sbk, sbn = c.N + o.get("pad_b", 0), 1
    return sam, sak, sbk, sbn


def gemm_args(c, A, B, Cm, bias=None, mask=None, gate=None, ws=None, mask_scale=2.0):
    """evacx.qnet.gemm_desc's arguments for a GEMM case: A, B, Cm the operands (anything with
    data_ptr(), Cm with .device too), bias / mask / gate given where the case's epilogue has them."""
    sam, sak, sbk, sbn = gemm_strides(c)
    o = c.opts
    assert ("b" in c.epi) == (bias is not None) and ("m" in c.epi) == (mask is not None)
    assert ("g" in c.epi) == (gate is not None)
    return dict(M=c.M, N=c.N, K=c.K, A=A, sam=sam, sak=sak, B=B, sbk=sbk, sbn=sbn, Cm=Cm,
                ldc=c.N + o.get("ldc_pad", 0), precision=c.prec, bias=bias, relu="r" in c.epi, mask=mask,
                ldm=c.N + 3, mask_scale=mask_scale, gate=gate, ldg=c.N + 5, accumulate="a" in c.epi,
                alpha=o.get("alpha", 1.0), ws=ws, split_ab=o.get("split_ab", False))


def gemm_ws(c, device):
    """The case's workspace argument: None, a _Workspace, or a tensor of f * M * N floats."""
    from evacx.qnet import _Workspace
    w = c.opts.get("ws")
    if w is None:
        return None
    return _Workspace() if w == "pool" else torch.empty(w * c.M * c.N, dtype=torch.float32, device=device)


def conv_dims(c):
    """(mode constant, M, N, K, cs) of a conv case."""
    from evacx import qnet
    Mp = c.B * 121
    if c.mode == "fwd":
        return qnet.CONV_FWD, Mp, c.cout, 9 * c.cin, c.cin
    if c.mode == "dx":
        return qnet.CONV_DX, Mp, c.cin, 9 * c.cout, c.cout
    return qnet.CONV_DW, c.cout, 9 * c.cin, Mp, c.cin


def conv_args(c, A, B, Cm, bias=None, gate=None, ws=None):
    """evacx.qnet.conv_desc's arguments for a conv case: forward A = X [B*121][cin], B = W; dX A = dY
    [B*121][cout], B = W, gate the layer below's output; dW A = dY, B = X."""
    mode, M, N, K, cs = conv_dims(c)
    kw = dict(mode=mode, M=M, N=N, K=K, A=A, B=B, Cm=Cm, cs=cs, ws=ws, out_split=c.opts.get("out_split", False))
    if c.mode == "fwd":
        kw.update(sbk=9, sbn=9 * c.cin, bias=bias, relu=True)
    elif c.mode == "dx":
        assert bool(c.opts.get("gate")) == (gate is not None)
        kw.update(sbk=9 * c.cin, sbn=9, gate=gate, ldg=c.cin)
    else:
        kw.update(sam=1, sak=c.cout)
    return kw


def check_plan(c, plan):
    """The launcher's plan for the case's descriptor is the one the case names."""
    from evacx._lib import REDUCE, ROUTE
    names = {v: k for k, v in ROUTE.items()}
    got = (names.get(plan.route, plan.route), plan.slices, {v: k for k, v in REDUCE.items()}[plan.reduce])
    assert got == (c.route, c.slices, c.reduce), (c.name, got, plan.klen)
    if "klen" in c.opts:
        assert plan.klen == c.opts["klen"], (c.name, plan.klen)
    assert plan.klen % 32 == 0 and plan.klen * plan.slices >= (c.K if isinstance(c, GemmCase) else conv_dims(c)[3])
