"""Plain references for the dense learner's small kernels (csrc/qnet.hip: evx_im2col3x3,
evx_col2im3x3, evx_pix_nchw, evx_pix_split, evx_relu_grad, evx_gather_obs, evx_sumsq_norm,
evx_colsum, evx_polyak, evx_clip_adam), in float64 or exact indexing, plus the inputs the CPU
and GPU tests share. Nothing here imports evacx: tests/test_qnet_helpers_cpu.py holds these
references to account against torch's own unfold / fold / clip_grad_norm_ / Adam, and
tests/test_qnet_helpers_gpu.py holds the kernels to these.

The clip + Adam step is restated twice: adam_ref_f64 (the formulas of clip_grad_norm_ and
torch.optim.Adam in float64, from the float32 inputs) and adam_ref_f32 (clip_adam_kernel op
for op in numpy float32, every operation rounded once, no fused multiply-add). The distance
of the second from the first, in units of 2^-24 of adam_scales, is the K the GPU test allows
(doubled): measured here, on the CPU, never from the kernel's output.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24  # unit roundoff of float32
GUARD = 256     # sentinel elements on each side of every output


# ------------------------------------------------------------------ guard bands
_SENTINEL = {torch.float32: 7777.0, torch.uint8: 0xA5, torch.int32: -0x5A5A5A5B, torch.int16: 0x5A5A}


def guarded(n, dtype=torch.float32, device="cuda"):
    """(whole buffer, the n live elements): GUARD sentinel elements before and after."""
    full = torch.full((n + 2 * GUARD,), _SENTINEL[dtype], dtype=dtype, device=device)
    return full, full[GUARD:GUARD + n]


def guards_intact(full):
    s = _SENTINEL[full.dtype]
    return bool((full[:GUARD] == s).all().item()) and bool((full[-GUARD:] == s).all().item())


# ------------------------------------------------------------------ conv helpers
def unfold_ref(x_nchw):
    """im2col of 3x3, padding 1 on 11x11 maps: [B][C][11][11] -> [B*121][C*9], k = c*9 + ky*3 + kx
    (F.unfold's own channel order), float64."""
    B, C = x_nchw.shape[:2]
    u = F.unfold(x_nchw.double(), 3, padding=1)  # [B][C*9][121]
    return u.permute(0, 2, 1).reshape(B * 121, C * 9).contiguous()


def fold_ref(dcols, B, C):
    """The adjoint of unfold_ref: [B*121][C*9] -> [B][C][11][11], float64."""
    u = dcols.double().reshape(B, 121, C * 9).permute(0, 2, 1)
    return F.fold(u, (11, 11), 3, padding=1)


def pix_to_nchw_ref(src, B, C):
    """[B*121][C] pixel-major -> [B][C][121]."""
    return src.reshape(B, 121, C).permute(0, 2, 1).contiguous()


def nchw_to_pix_ref(src, B, C):
    """[B][C][121] -> [B*121][C] pixel-major."""
    return src.reshape(B, C, 121).permute(0, 2, 1).reshape(B * 121, C).contiguous()


def pix_split_ref(src, B, C):
    """NCHW [B][C][121] f32 -> the pixel-major bf16 planes [2][B][121*C] as int16 bit patterns:
    hi = round-to-nearest-even bf16 of x, lo = bf16 of the f32 remainder x - hi."""
    x = nchw_to_pix_ref(src.float(), B, C).reshape(B, 121 * C)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).view(torch.int16)


def split_inputs(B, C, seed):
    """[B][C][121] f32 for evx_pix_split: +-0, exact bf16 values (lo = 0), ties of the bf16 rounding
    (the dropped 16 bits are exactly 0x8000, on an even and on an odd kept mantissa), magnitudes
    2^-100 .. 2^100, and plain randn."""
    g = torch.Generator().manual_seed(seed)
    n = B * C * 121
    x = torch.randn(n, generator=g)
    e = torch.randint(-100, 101, (n,), generator=g).float()
    x = torch.where(torch.arange(n) % 3 == 0, x * torch.exp2(e), x)
    bits = x.view(torch.int32).clone()
    k = torch.arange(n) % 7
    bits = torch.where(k == 1, bits & ~0xFFFF, bits)                   # exact bf16
    bits = torch.where(k == 2, (bits & ~0x1FFFF) | 0x8000, bits)       # tie, kept mantissa even
    bits = torch.where(k == 3, (bits & ~0x1FFFF) | 0x18000, bits)      # tie, kept mantissa odd
    x = bits.view(torch.float32).clone()
    x[k == 4] = 0.0
    x[k == 5] = -0.0
    assert torch.isfinite(x).all()
    return x.reshape(B, C, 121)


def relu_grad_ref(dy, y):
    """dy where y > 0, else 0: a NaN y is not > 0, so it zeroes dy."""
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def relu_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, 2.0 ** -126, -2.0 ** -126, float("nan"), -1.0, 1.0])
    k = torch.arange(n) % 11
    for j in range(special.numel()):  # n = 1: the one element is +0
        y[k == j] = special[j]
    dy = torch.randn(n, generator=g) + 3.0  # away from 0: a kept element is never mistaken for a zeroed one
    return dy, y


def gather_ref(src, idx):
    """src: int32 [rows][8] (evx_obs rows), idx int64 [n]."""
    return src.view(-1, 8)[idx]


# ------------------------------------------------------------------ sums
def norm_ref(g):
    return float(g.double().pow(2).sum().sqrt())


def sumsq_parts(n, scratch_elems):
    """The partial sums evx_sumsq_norm's launcher takes: one per 4096 elements, at most the
    scratch and at most 2048, at least 1."""
    return max(1, min((n + 4095) // 4096, scratch_elems, 2048))


def sumsq_bound(n, scratch_elems):
    """Relative bound of the f32 norm: every term is >= 0, so a sum of T terms in any order is
    within T u of exact; a thread sums T = ceil(n / (256 parts)) squares, the block tree and the
    finish add ceil(parts / 256) + 16 more levels, the squares, the square root and the final
    rounding a few more: (T + ceil(parts / 256) + 20) u."""
    parts = sumsq_parts(n, scratch_elems)
    T = -(-n // (256 * parts))
    return (T + -(-parts // 256) + 20) * U


def colsum_ref(X, N, out0=None):
    """X: [M][ld] with ld >= N; the first N columns summed over rows in float64 (+ out0)."""
    s = X[:, :N].double().sum(0)
    return s if out0 is None else s + out0.double()


# ------------------------------------------------------------------ polyak
def polyak_ref_f32(p, t, tau, omt):
    """t' = tau * p + omt * t in float32: two products and a sum, each rounded once (the library
    is built without contraction, so no fused multiply-add: one IEEE result)."""
    p, t = np.asarray(p, np.float32), np.asarray(t, np.float32)
    a = np.float32(tau) * p
    b = np.float32(omt) * t
    return (a + b).astype(np.float32)


# ------------------------------------------------------------------ clip + Adam
class AdamHyper:
    """evx_adam's fields as the float32 values the library receives, and the two scalars
    evx_clip_adam derives on the host in double before rounding them to float32."""

    def __init__(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1):
        self.lr, self.beta1, self.beta2 = np.float32(lr), np.float32(beta1), np.float32(beta2)
        self.eps, self.weight_decay, self.step = np.float32(eps), np.float32(weight_decay), int(step)
        self.bc1 = 1.0 - float(self.beta1) ** self.step
        self.bc2 = 1.0 - float(self.beta2) ** self.step
        self.step_size = np.float32(float(self.lr) / self.bc1)
        self.bc2_sqrt = np.float32(math.sqrt(self.bc2))


def clip_coef64(norm, max_norm):
    """clip_grad_norm_'s coefficient max_norm / (norm + 1e-6), clamped to 1 (1e-6 as the float32
    constant the kernel adds); 1 when there is no norm or max_norm is not positive."""
    if norm is None or not max_norm > 0:
        return 1.0
    return min(float(np.float32(max_norm)) / (float(np.float32(norm)) + float(np.float32(1e-6))), 1.0)


def adam_step64(p, g, m, v, coef, beta1, beta2, eps, wd, step_size, bc2_sqrt):
    """clip_grad_norm_'s scaling by coef, then torch.optim.Adam's single-tensor update, on float64
    arrays. Returns (p, g, m, v, denom) -- g as the optimizer uses it, clipped and with the weight
    decay term -- and the clipped gradient before that term."""
    gc = g * coef                                   # clip_grad_norm_: g.mul_(clip_coef_clamped)
    gi = gc + wd * p if wd != 0.0 else gc           # grad.add(param, alpha=weight_decay)
    mi = m + (gi - m) * (1.0 - beta1)               # exp_avg.lerp_(grad, 1 - beta1)
    vi = v * beta2 + (1.0 - beta2) * gi * gi        # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    denom = np.sqrt(vi) / bc2_sqrt + eps            # (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    pi = p - step_size * (mi / denom)               # param.addcdiv_(exp_avg, denom, value=-step_size)
    return (pi, gi, mi, vi, denom), gc


def adam_ref_f64(p, g, m, v, norm, max_norm, h):
    """adam_step64 from the float32 inputs of one evx_clip_adam call: the arrays, the norm and the
    hyper-parameters widened exactly; the step size and sqrt(bias correction 2) are the float32
    scalars the launcher hands the kernel."""
    p, g, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    return adam_step64(p, g, m, v, clip_coef64(norm, max_norm), float(h.beta1), float(h.beta2), float(h.eps),
                       float(h.weight_decay), float(h.step_size), float(h.bc2_sqrt))


def adam_ref_f32(p, g, m, v, norm, max_norm, h):
    """clip_adam_kernel op for op in numpy float32 (each operation rounded once)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    coef = f(1.0)
    if norm is not None and f(max_norm) > f(0.0):
        coef = f(max_norm) / (f(norm) + f(1e-6))
        coef = coef if coef < f(1.0) else f(1.0)
    gi = g * coef
    if h.weight_decay != f(0.0):
        gi = gi + h.weight_decay * p
    mi = m + (gi - m) * (f(1.0) - h.beta1)
    vi = v * h.beta2 + ((f(1.0) - h.beta2) * gi) * gi
    denom = np.sqrt(vi) / h.bc2_sqrt + h.eps
    pi = p - h.step_size * (mi / denom)
    for a in (pi, gi, mi, vi):
        assert a.dtype == np.float32
    return pi, gi, mi, vi


def adam_scales(p0, g_clipped, ref, h):
    """Per-element magnitudes the float32 error is measured in (x 2^-24), from the float64
    reference: for p the parameter plus the size of its update's operands,
    |p| + step_size (|m| + |g|) / denom.
    With weight decay g = coef g0 + wd p can cancel, and m = m0 + (g - m0)(1 - beta1) can: the
    rounding of the operands then stays the size of the operands, not of the small result (measured
    on the CPU: against the plain |g|, |m| the float32 restatement itself is 5e4 and 2e6 units
    off at the worst cancellations of these inputs). So, as the p scale adds |g| to |m|, the
    scales of g, m and v carry the operands: gs = |coef g0| + wd |p0| for g (the plain |g| without
    weight decay), |m| + gs for m, and v + (1 - beta2) gs^2 for v."""
    pi, gi, mi, vi, denom = ref
    p0 = np.asarray(p0, np.float32).astype(np.float64)
    sp = np.abs(pi) + float(h.step_size) * (np.abs(mi) + np.abs(gi)) / denom
    gs = np.abs(g_clipped) + float(h.weight_decay) * np.abs(p0)
    return dict(p=sp, g=gs, m=np.abs(mi) + gs, v=np.abs(vi) + (1.0 - float(h.beta2)) * gs * gs)


def adam_units(got, p0, g_clipped, ref, h):
    """max over elements and over p, g, m, v of |got - ref| / (2^-24 scale): the K that `got`
    needs. Where the scale is 0 the result must be exactly the reference (inf otherwise)."""
    sc = adam_scales(p0, g_clipped, ref, h)
    worst = 0.0
    for name, a, r in zip("pgmv", got, ref):
        err = np.abs(np.asarray(a, np.float64) - r)
        s = sc[name] * U
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(s > 0, err / s, np.where(err == 0, 0.0, np.inf))
        worst = max(worst, float(k.max()))
    return worst


# The measured K (tests/test_qnet_helpers_cpu.py::test_adam_f32_restatement_meets_K asserts it):
# the float32 restatement is within ADAM_K_CPU * 2^-24 * scale of the float64 reference on every
# input of adam_cases(). The GPU bound is twice that (its divide and sqrt may round the last bit
# the other way).
ADAM_K_CPU = 8
ADAM_K_GPU = 2 * ADAM_K_CPU

ADAM_SMALL = (1, 255, 257)
ADAM_LARGE = (4096 * 256 + 3, 2 * 4096 * 256 + 1)  # one element past one grid pass, and past two
ADAM_NORM_MODES = ("null", "max0", "below", "above")


def adam_inputs(n, seed):
    """p, g, m, v float32 [n]: gradients of mixed sign spread over 1e-12 .. 1, every 8th element
    g = 0 with v = 0 (the denominator is eps alone; m = 0 too on every 16th)."""
    r = np.random.RandomState(seed)
    p = (r.randn(n) * 0.1).astype(np.float32)
    g = (r.randn(n) * 10.0 ** r.uniform(-12, 0, n)).astype(np.float32)
    m = (r.randn(n) * 1e-3).astype(np.float32)
    v = ((r.randn(n) * 1e-3) ** 2).astype(np.float32)
    i = np.arange(n)
    if n > 1:
        g[i % 8 == 3] = 0
        v[i % 8 == 3] = 0
        m[i % 16 == 3] = 0
        g[i % 8 == 5] = np.float32(1e-12) * np.where(i[i % 8 == 5] % 16 == 5, 1, -1)
    return p, g, m, v


def adam_case(n, mode, wd, step, betas, seed):
    """One test case: the inputs, the norm the kernel is given (the gradient's own float32 norm,
    or None) and max_norm so that the norm lies below or above it."""
    p, g, m, v = adam_inputs(n, seed)
    h = AdamHyper(lr=1e-3, beta1=betas[0], beta2=betas[1], eps=1e-8, weight_decay=wd, step=step)
    gn = np.float32(math.sqrt(float((g.astype(np.float64) ** 2).sum())))
    norm, max_norm = gn, 1.0
    if mode == "null":
        norm = None
    elif mode == "max0":
        max_norm = 0.0
    elif mode == "below":
        max_norm = float(np.float32(2.0 * float(gn) + 1.0))
    else:
        assert mode == "above"
        max_norm = float(np.float32(0.37 * float(gn)))
    return dict(n=n, mode=mode, p=p, g=g, m=m, v=v, norm=norm, max_norm=max_norm, h=h)


def adam_cases(sizes=None):
    """Every case of the GPU test: the small sizes crossed with the norm modes, weight decay,
    steps and betas; each large size with the four norm modes (the other options alternating)."""
    seed = 0
    for n in ADAM_SMALL:
        if sizes is not None and n not in sizes:
            continue
        for mode in ADAM_NORM_MODES:
            for wd in (0.0, 0.01):
                for step in (1, 2, 1000):
                    for betas in ((0.9, 0.999), (0.8, 0.99)):
                        seed += 1
                        yield adam_case(n, mode, wd, step, betas, 1000 * n + seed)
    for n in ADAM_LARGE:
        if sizes is not None and n not in sizes:
            continue
        for j, mode in enumerate(ADAM_NORM_MODES):
            yield adam_case(n, mode, (0.0, 0.01)[j % 2], (1, 2, 1000, 2)[j], ((0.9, 0.999), (0.8, 0.99))[j // 2],
                            n % 9973 + j)


def adam_clips(c):
    """Whether the case's coefficient is below 1 (the gradient is scaled)."""
    return clip_coef64(c["norm"], c["max_norm"]) < 1.0
