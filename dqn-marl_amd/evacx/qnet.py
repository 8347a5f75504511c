"""Device Q-networks and the DQN learner step (host driver of libevacx's learner kernels).

Reference: Louvre_Evacuation/agents/dqn_agent.py
  * DQNNetwork (:15-61): conv 6->32->64->128 (3x3, pad 1) on the 11x11x6 patch,
    fc 15488->512 (+ReLU, Dropout 0.2) ->256 (+ReLU) ->5.     -> ``ConvQNet``
  * the build-defined MLP variant for the vectorised configs:
    726->512 (+ReLU, Dropout) ->256 (+ReLU) ->5.              -> ``MLPQNet``
  * DQNAgent.learn (:126-168): Q(s).gather(a), r + gamma max Q_tgt(s') ~done, MSE,
    backward, clip_grad_norm_(1.0), Adam.                      -> ``Learner.learn``

Parameters, gradients and Adam moments each live in ONE flat fp32 buffer (the
reference's state_dict order), so clip+Adam is one fused kernel and a multi-GPU
gradient all-reduce is one collective. Every contraction runs in evx_gemm
(MFMA); torch only allocates.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch

from ._lib import (ACCUM, CONV_DW, CONV_DX, CONV_FWD, OUT_SPLIT, PREC, RELU, SPLIT_AB, check,  # noqa: F401
                   evx_adam, evx_gemm_desc, evx_gemm_plan, lib)
from .env import _stream
from .qmlp import (evx_td_opts, polyak_coeffs, td_opts, validate_nets_options,  # noqa: F401 (re-exported)
                   validate_td_options)

DROPOUT_P = 0.2
# the loader's and the check's earlier names here, kept for callers written against them
qlib, qcheck = lib, check


def _p(t):
    return None if t is None else t.data_ptr()


def td_workspace(ws, B: int, nets: int, device, tag: str = "") -> torch.Tensor:
    """The TD loss's partials buffer (evx_td_loss_ws_floats) from a _Workspace pool."""
    n = max(1, int(lib().evx_td_loss_ws_floats(B, nets)))
    return ws.get(tag + "td_ws", (n,), torch.float32, device)


_WS_NEED: Dict[Tuple, int] = {}


def _attach_ws(d, ws, tag, device, conv=None):
    """Workspace of a descriptor (evx_gemm_ws_elems: split-K partials; conv = (mode, channels):
    evx_conv3x3_ws_elems, which also covers the conv forward's packed weights): ws is a _Workspace
    (a buffer per tag and size, kept for the pool's life, so a stream never sees another stream's
    scratch freed or rewritten under it), a f32 tensor, or None (the GEMM runs in one pass)."""
    if ws is None:
        return
    key = (d.M, d.N, d.K, d.precision, d.flags, bool(d.bias), bool(d.mask), bool(d.gate), d.sbk, d.sbn, conv)
    need = _WS_NEED.get(key)
    if need is None:
        need = _WS_NEED[key] = int(lib().evx_conv3x3_ws_elems(C.byref(d), conv[0], conv[1]) if conv
                                   else lib().evx_gemm_ws_elems(C.byref(d)))
    if need <= 0:
        return
    if isinstance(ws, torch.Tensor):
        if ws.dtype != torch.float32:
            raise ValueError("gemm workspace must be float32")
        d.ws, d.ws_elems = ws.data_ptr(), ws.numel()
        return
    buf = ws.get(tag + "splitk", (need,), torch.float32, device)
    d.ws, d.ws_elems = buf.data_ptr(), need


def gemm_desc(M, N, K, A, sam, sak, B, sbk, sbn, Cm, ldc, precision="f32", bias=None, relu=False, mask=None,
              ldm=0, mask_scale=1.0, gate=None, ldg=0, accumulate=False, alpha=1.0, ws=None, tag="", split_ab=False):
    """The descriptor of an evx_gemm call, its workspace attached (gemm's arguments)."""
    d = evx_gemm_desc(M=M, N=N, K=K, precision=PREC[precision],
                      flags=(RELU if relu else 0) | (ACCUM if accumulate else 0) | (SPLIT_AB if split_ab else 0),
                      alpha=alpha, A=_p(A), sam=sam, sak=sak, B=_p(B), sbk=sbk, sbn=sbn, C=_p(Cm), ldc=ldc,
                      bias=_p(bias), mask=_p(mask), ldm=ldm, mask_scale=mask_scale, gate=_p(gate), ldg=ldg)
    _attach_ws(d, ws, tag, Cm.device)
    return d


def gemm(*args, **kw):
    """evx_gemm (gemm_desc's arguments); split_ab: A and B are bf16 hi / lo planes (int16 tensors, x3,
    k-contiguous)."""
    check(lib().evx_gemm(C.byref(gemm_desc(*args, **kw)), _stream()), "evx_gemm")


def conv_desc(mode, M, N, K, A, B, Cm, cs, sam=0, sak=0, sbk=0, sbn=0, bias=None, relu=False, gate=None,
              ldg=0, ws=None, tag="", out_split=False):
    """The descriptor of an evx_conv3x3_gemm call, its workspace attached (conv_gemm's arguments)."""
    d = evx_gemm_desc(M=M, N=N, K=K, precision=PREC["x3"], flags=(RELU if relu else 0) | (OUT_SPLIT if out_split else 0),
                      alpha=1.0, A=_p(A),
                      sam=sam, sak=sak, B=_p(B), sbk=sbk, sbn=sbn, C=_p(Cm), ldc=N, bias=_p(bias), mask=None,
                      ldm=0, mask_scale=1.0, gate=_p(gate), ldg=ldg)
    _attach_ws(d, ws, tag + f"cv{mode}_", Cm.device, conv=(mode, cs))
    return d


def conv_gemm(mode, M, N, K, A, B, Cm, cs, **kw):
    """evx_conv3x3_gemm (x3): implicit-GEMM 3x3 conv forward / dX / dW on pixel-major activations
    (conv_desc's arguments). out_split: the output as bf16 hi / lo planes (Cm int16 [2][M][N]; the
    LDS-staged forward)."""
    d = conv_desc(mode, M, N, K, A, B, Cm, cs, **kw)
    check(lib().evx_conv3x3_gemm(C.byref(d), mode, cs, _stream()), "evx_conv3x3_gemm")


def gemm_plan(d, mode=0, cs=0):
    """evx_gemm_plan_query: the kernel route, K slices, slice length and reduction the launcher would
    take for descriptor d (mode 0: evx_gemm; CONV_*: evx_conv3x3_gemm(mode, cs)). Host only."""
    p = evx_gemm_plan()
    check(lib().evx_gemm_plan_query(C.byref(d), mode, cs, C.byref(p)), "evx_gemm_plan_query")
    return p


def colsum(X, M, N, out, scratch):
    check(lib().evx_colsum(_p(X), N, M, N, _p(out), 0, _p(scratch), scratch.numel(), _stream()), "evx_colsum")


# ----------------------------------------------------------------------------
# parameter layout
# ----------------------------------------------------------------------------
def layer_specs(kind: str, hidden: int = 512, actions: int = 5, in_dim: int = 726) -> List[Tuple]:
    """(name, type, fan_in, fan_out[, conv channels]) in the reference state_dict order."""
    if kind == "conv":
        return [("conv1", "conv", 6, 32), ("conv2", "conv", 32, 64), ("conv3", "conv", 64, 128),
                ("fc1", "fc", 11 * 11 * 128, hidden), ("fc2", "fc", hidden, hidden // 2),
                ("fc3", "fc", hidden // 2, actions)]
    if kind == "mlp":
        return [("fc1", "fc", in_dim, hidden), ("fc2", "fc", hidden, hidden // 2),
                ("fc3", "fc", hidden // 2, actions)]
    raise ValueError(kind)


def param_shapes(specs) -> "OrderedDict[str, Tuple[int, ...]]":
    out = OrderedDict()
    for name, typ, fi, fo in specs:
        out[name + ".weight"] = (fo, fi, 3, 3) if typ == "conv" else (fo, fi)
        out[name + ".bias"] = (fo,)
    return out


class FlatParams:
    """All tensors of one network in one flat fp32 device buffer (state_dict order)."""

    def __init__(self, shapes, device, data: Optional[torch.Tensor] = None):
        self.shapes = shapes
        self.numel = sum(int(torch.Size(s).numel()) for s in shapes.values())
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=device) if data is None else data
        self.views: Dict[str, torch.Tensor] = OrderedDict()
        o = 0
        for k, s in shapes.items():
            n = int(torch.Size(s).numel())
            self.views[k] = self.flat[o:o + n].view(s)
            o += n

    def __getitem__(self, k):
        return self.views[k]

    def state_dict(self):
        return OrderedDict((k, v.detach().clone()) for k, v in self.views.items())

    def load_state_dict(self, sd):
        for k, v in self.views.items():
            v.copy_(sd[k].to(v.device, torch.float32).view(v.shape))

    def init_from_global_torch(self):
        """The reference's own initialisation: each layer's nn.Conv2d / nn.Linear
        reset_parameters (kaiming_uniform_(w, a=sqrt(5)), then bias ~ U(+-1/sqrt(fan_in)))
        drawn from torch's global CPU generator in state_dict order, so after
        torch.manual_seed(s) the weights and the generator's position equal a freshly built
        reference DQNNetwork's (agents/dqn_agent.py:22-31)."""
        import math
        for k, v in self.views.items():
            if k.endswith(".weight"):
                w = torch.empty(self.shapes[k])
                torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5))
                v.copy_(w)
            else:
                ws = self.shapes[k[:-5] + ".weight"]
                fan_in = ws[1] * (ws[2] * ws[3] if len(ws) == 4 else 1)
                bound = 1.0 / math.sqrt(fan_in) if fan_in > 0 else 0.0
                v.copy_(torch.empty(self.shapes[k]).uniform_(-bound, bound))

    def init_like_torch(self, seed: int):
        """nn.Conv2d / nn.Linear default init (kaiming_uniform a=sqrt(5) -> U(+-1/sqrt(fan_in)))."""
        g = torch.Generator().manual_seed(seed)
        for k, v in self.views.items():
            w_name = k[:-5] + ".weight" if k.endswith(".bias") else k
            ws = self.shapes[w_name]
            fan_in = ws[1] * (ws[2] * ws[3] if len(ws) == 4 else 1)
            bound = 1.0 / (fan_in ** 0.5)
            v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) * bound)


# ----------------------------------------------------------------------------
# networks
# ----------------------------------------------------------------------------
class _Workspace:
    def __init__(self):
        self.bufs: Dict[Tuple, torch.Tensor] = {}

    def get(self, name, shape, dtype, device):
        key = (name, tuple(shape), dtype)
        t = self.bufs.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=device)
            self.bufs[key] = t
        return t


class QNet:
    """Forward/backward of the reference DQNNetwork (or the MLP variant) on evx_gemm."""

    def __init__(self, kind: str, params: FlatParams, precision="f32", hidden=512, actions=5):
        self.kind, self.P, self.prec = kind, params, precision
        self.hidden, self.actions = hidden, actions
        # x3 conv layers as implicit GEMMs (the exact-f32 path keeps im2col + GEMM)
        self.implicit = kind == "conv" and precision == "x3"
        self.device = params.flat.device
        self.ws = _Workspace()
        self.saved = None

    # ------------------------------------------------------------ fc stack
    def _fc_forward(self, X, B, K0, mask, tag, w1=None, split=False):
        """split: X and w1 are bf16 hi / lo planes (int16 [2][B][K0], [2][H][K0]) -- the act's fc1."""
        P, ws, dev, H, A = self.P, self.ws, self.device, self.hidden, self.actions
        H1 = ws.get(tag + "h1", (B, H), torch.float32, dev)
        gemm(B, H, K0, X, K0, 1, P["fc1.weight"] if w1 is None else w1, 1, K0, H1, H, self.prec, bias=P["fc1.bias"],
             relu=True,
             mask=mask, ldm=H, mask_scale=1.0 / (1.0 - DROPOUT_P), ws=self.ws, tag=tag, split_ab=split)
        H2 = ws.get(tag + "h2", (B, H // 2), torch.float32, dev)
        gemm(B, H // 2, H, H1, H, 1, P["fc2.weight"], 1, H, H2, H // 2, self.prec, bias=P["fc2.bias"], relu=True, ws=self.ws, tag=tag)
        Q = ws.get(tag + "q", (B, A), torch.float32, dev)
        gemm(B, A, H // 2, H2, H // 2, 1, P["fc3.weight"], 1, H // 2, Q, A, self.prec, bias=P["fc3.bias"], ws=self.ws, tag=tag)
        return H1, H2, Q

    def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor], save=True, tag="") -> torch.Tensor:
        """x: [B, 11, 11, 6] (or [B, 726]) fp32; mask: [B, hidden] uint8 dropout keep-mask or None (eval)."""
        B = x.shape[0]
        x = x.reshape(B, -1).contiguous()
        if self.kind == "mlp":
            H1, H2, Q = self._fc_forward(x, B, x.shape[1], mask, tag)
            if save:
                self.saved = dict(B=B, x=x, H1=H1, H2=H2, mask=mask)
            return Q
        ws, dev, P = self.ws, self.device, self.P
        L = lib()
        Mp = B * 121
        ins, cols, ys = [x], [], []
        cur, C_in = x, 6
        # without saves (the act): conv3's output leaves as bf16 hi / lo planes and fc1 runs on
        # pre-split operands (EVX_GEMM_SPLIT_AB: its K tiles staged as 16-B copies)
        split = self.implicit and not save
        for li, (cname, cout) in enumerate([("conv1", 32), ("conv2", 64), ("conv3", 128)]):
            K9 = C_in * 9
            if self.implicit:  # x3: the taps gathered in the GEMM's tile fetch (no im2col buffer)
                osp = split and li == 2
                Y = ws.get(tag + f"y{li}" + ("s" if osp else ""), (2 * Mp, cout) if osp else (Mp, cout),
                           torch.int16 if osp else torch.float32, dev)
                conv_gemm(CONV_FWD, Mp, cout, K9, cur, P[cname + ".weight"], Y, C_in, sbk=9, sbn=K9,
                          bias=P[cname + ".bias"], relu=True, ws=self.ws, tag=tag, out_split=osp)
                cols.append(cur)  # the layer input, gathered again by the dW GEMM
                ys.append(Y)
                cur, C_in = Y, cout
                continue
            col = ws.get(tag + f"col{li}", (Mp, K9), torch.float32, dev)
            check(L.evx_im2col3x3(_p(cur), B, C_in, 1, _p(col), _stream()), "im2col")
            Y = ws.get(tag + f"y{li}", (Mp, cout), torch.float32, dev)
            gemm(Mp, cout, K9, col, K9, 1, P[cname + ".weight"], 1, K9, Y, cout, self.prec, bias=P[cname + ".bias"],
                 relu=True, ws=self.ws, tag=tag)
            cols.append(col)
            ys.append(Y)
            cur, C_in = Y, cout
        if self.implicit:
            # fc1 reads conv3's pixel-major output as it lies ([B][121 * 128], column p * 128 + c)
            # against a copy of fc1.weight with its columns in that order (the reference flattens
            # NCHW: column c * 121 + p). The copy is made per forward (31.7 MB, ~20 us) instead of
            # transposing the activations (8192 rows: 507 MB, 0.57 ms).
            if split:
                W1s = ws.get(tag + "w1s", (2 * self.hidden, 128 * 121), torch.int16, dev)
                check(L.evx_pix_split(_p(P["fc1.weight"]), self.hidden, 128, _p(W1s), _stream()), "pix_split")
                _, _, Q = self._fc_forward(cur, B, 128 * 121, mask, tag, w1=W1s, split=True)
                return Q
            W1p = ws.get(tag + "w1p", (self.hidden, 128 * 121), torch.float32, dev)
            check(L.evx_pix_nchw(_p(P["fc1.weight"]), self.hidden, 128, 0, _p(W1p), _stream()), "pix_nchw")
            F = cur.view(B, 128 * 121)
            H1, H2, Q = self._fc_forward(F, B, 128 * 121, mask, tag, w1=W1p)
            if save:
                self.saved = dict(B=B, x=F, H1=H1, H2=H2, mask=mask, cols=cols, ys=ys, w1p=W1p)
            return Q
        F = ws.get(tag + "flat", (B, 128 * 121), torch.float32, dev)
        check(L.evx_pix_nchw(_p(cur), B, 128, 1, _p(F), _stream()), "pix_nchw")  # torch reshape of NCHW
        H1, H2, Q = self._fc_forward(F, B, 128 * 121, mask, tag)
        if save:
            self.saved = dict(B=B, x=F, H1=H1, H2=H2, mask=mask, cols=cols, ys=ys)
        return Q

    def backward(self, dQ: torch.Tensor, grads: FlatParams):
        """Writes d loss / d params into `grads` (overwrites) for the saved forward."""
        s = self.saved
        assert s is not None, "forward(save=True) first"
        B, X, H1, H2, mask = s["B"], s["x"], s["H1"], s["H2"], s["mask"]
        P, ws, dev, H, A, pr = self.P, self.ws, self.device, self.hidden, self.actions, self.prec
        K0 = X.shape[1]
        # colsum partials: one per 64 rows and column (evx_colsum)
        scratch = ws.get("colsum", (max(1, (max(B * 121, B) + 63) // 64) * max(H, 128),), torch.float32, dev)
        # fc3
        gemm(A, H // 2, B, dQ, 1, A, H2, H // 2, 1, grads["fc3.weight"], H // 2, pr, ws=self.ws, tag="bw_")
        colsum(dQ, B, A, grads["fc3.bias"], scratch)
        dZ2 = ws.get("dz2", (B, H // 2), torch.float32, dev)
        gemm(B, H // 2, A, dQ, A, 1, P["fc3.weight"], H // 2, 1, dZ2, H // 2, pr, gate=H2, ldg=H // 2, ws=self.ws, tag="bw_")
        # fc2
        gemm(H // 2, H, B, dZ2, 1, H // 2, H1, H, 1, grads["fc2.weight"], H, pr, ws=self.ws, tag="bw_")
        colsum(dZ2, B, H // 2, grads["fc2.bias"], scratch)
        dZ1 = ws.get("dz1", (B, H), torch.float32, dev)
        gemm(B, H, H // 2, dZ2, H // 2, 1, P["fc2.weight"], H, 1, dZ1, H, pr, mask=mask, ldm=H,
             mask_scale=1.0 / (1.0 - DROPOUT_P), gate=H1, ldg=H, ws=self.ws, tag="bw_")
        # fc1
        L = lib()
        W1p = s.get("w1p")
        if W1p is None:
            gemm(H, K0, B, dZ1, 1, H, X, K0, 1, grads["fc1.weight"], K0, pr, ws=self.ws, tag="bw_")
        else:  # X is pixel-major: dW1 in that column order, then back to the reference's
            dW1p = ws.get("dw1p", (H, K0), torch.float32, dev)
            gemm(H, K0, B, dZ1, 1, H, X, K0, 1, dW1p, K0, pr, ws=self.ws, tag="bw_")
            check(L.evx_pix_nchw(_p(dW1p), H, 128, 1, _p(grads["fc1.weight"]), _stream()), "pix_nchw")
        colsum(dZ1, B, H, grads["fc1.bias"], scratch)
        if self.kind == "mlp":
            return
        Mp = B * 121
        dY = ws.get("dy2", (Mp, 128), torch.float32, dev)
        if W1p is not None:  # dF in pixel order is conv3's dY
            gemm(B, K0, H, dZ1, H, 1, W1p, K0, 1, dY.view(B, K0), K0, pr, gate=X, ldg=K0, ws=self.ws, tag="bw_")
        else:
            dF = ws.get("dflat", (B, K0), torch.float32, dev)
            gemm(B, K0, H, dZ1, H, 1, P["fc1.weight"], K0, 1, dF, K0, pr, gate=X, ldg=K0, ws=self.ws, tag="bw_")  # gate: relu(conv3) > 0
            check(L.evx_pix_nchw(_p(dF), B, 128, 0, _p(dY), _stream()), "pix_nchw")
        cols, ys = s["cols"], s["ys"]
        for li, (cname, cin, cout) in reversed(list(enumerate([("conv1", 6, 32), ("conv2", 32, 64),
                                                                ("conv3", 64, 128)]))):
            K9 = cin * 9
            if self.implicit:  # cols[li] is the layer input [Mp][cin]
                conv_gemm(CONV_DW, cout, K9, Mp, dY, cols[li], grads[cname + ".weight"], cin, sam=1, sak=cout, ws=self.ws, tag="bw_")
                colsum(dY, Mp, cout, grads[cname + ".bias"], scratch)
                if li == 0:
                    break
                dYp = ws.get(f"dyp{li}", (Mp, cin), torch.float32, dev)
                conv_gemm(CONV_DX, Mp, cin, cout * 9, dY, P[cname + ".weight"], dYp, cout, sbk=K9, sbn=9,
                          gate=ys[li - 1], ldg=cin, ws=self.ws, tag="bw_")
                dY = dYp
                continue
            gemm(cout, K9, Mp, dY, 1, cout, cols[li], K9, 1, grads[cname + ".weight"], K9, pr, ws=self.ws, tag="bw_")
            colsum(dY, Mp, cout, grads[cname + ".bias"], scratch)
            if li == 0:
                break
            dcol = ws.get(f"dcol{li}", (Mp, K9), torch.float32, dev)
            gemm(Mp, K9, cout, dY, cout, 1, P[cname + ".weight"], K9, 1, dcol, K9, pr, ws=self.ws, tag="bw_")
            dx = ws.get(f"dx{li}", (B, cin * 121), torch.float32, dev)
            check(L.evx_col2im3x3(_p(dcol), B, cin, _p(dx), _stream()), "col2im")
            dYp = ws.get(f"dyp{li}", (Mp, cin), torch.float32, dev)
            check(L.evx_pix_nchw(_p(dx), B, cin, 0, _p(dYp), _stream()), "pix_nchw")
            check(L.evx_relu_grad(_p(dYp), _p(ys[li - 1]), dYp.numel(), _stream()), "relu_grad")
            dY = dYp


class Learner:
    """Online + target networks, fused clip+Adam, TD loss: DQNAgent.learn on the device."""

    def __init__(self, kind="mlp", device="cuda", lr=1e-4, gamma=0.99, max_norm=1.0, precision="f32",
                 hidden=512, actions=5, seed=0, betas=(0.9, 0.999), eps=1e-8, double_q=False, loss="mse",
                 huber_delta=1.0, target_tau=0.0, stats=None):
        """stats: an evacx.lstats.LearnStats of 1 net, or None: every step_optimizer() ends with one
        stats.update of the learn step's batch on its stream (the learner's numbers do not change).
        double_q: the target bootstraps from the target net's value of the online net's greedy
        action at s' (one more online forward per learn step); loss: "mse" or "huber" (with
        huber_delta); target_tau > 0: soft_update() blends the target towards the online net.
        None of them is the reference's; all off is DQNAgent.learn."""
        validate_td_options(loss, huber_delta, target_tau)
        self.double_q, self.loss_kind = bool(double_q), loss
        self.huber_delta, self.target_tau = float(huber_delta), float(target_tau)
        self.last_sel = None  # double_q: the last learn step's bootstrap actions (int32 [B], device)
        self._sel_ws = {}     # the selection act's workspaces by batch size
        if stats is not None and (getattr(stats, "nets", None) != 1 or stats.A != actions):
            raise ValueError(f"Learner: stats must be a LearnStats of 1 net and A = {actions}")
        self.stats = stats
        self.stat_batch = None  # stats: (Q, Qt, a, r, done, sel, gamma_row, B) of the last learn step
        if precision not in ("f32", "bf16", "x3", "exact"):
            raise ValueError(f"precision must be 'f32', 'bf16', 'x3' or 'exact', not {precision!r}")
        # "exact": every product on the exact-f32 MFMA GEMMs (evx_gemm f32), no fused MLP kernels
        fused_ok = precision != "exact"
        precision = "f32" if precision == "exact" else precision
        self.kind, self.device = kind, torch.device(device)
        self.shapes = param_shapes(layer_specs(kind, hidden, actions))
        self.online = FlatParams(self.shapes, self.device)
        self.online.init_like_torch(seed)
        self.target = FlatParams(self.shapes, self.device)
        self.target.flat.copy_(self.online.flat)
        self.grads = FlatParams(self.shapes, self.device)
        self.m = torch.zeros_like(self.online.flat)
        self.v = torch.zeros_like(self.online.flat)
        self.adam_step = 0
        self.lr, self.gamma, self.max_norm, self.betas, self.eps = lr, gamma, max_norm, betas, eps
        self.hidden, self.actions, self.precision = hidden, actions, precision
        self.net = QNet(kind, self.online, precision, hidden, actions)
        self.tnet = QNet(kind, self.target, precision, hidden, actions)
        self.norm = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.scratch = torch.zeros(2048, dtype=torch.float32, device=self.device)
        self.seed = seed
        self.rng_offset = 0
        self.grad_hook = None  # e.g. an all-reduce over the flat grad buffer
        # MLP: the fused kernels of csrc/qmlp.hip (forward from compact observations); f32 runs
        # them in the x3 (f32-accurate) mode, bf16 with bf16 operands. The dense-tensor path
        # (forward / learn on expanded observations) keeps evx_gemm at `precision`.
        self.fast = self.fast_t = None
        if fused_ok and kind == "mlp" and hidden == 512 and actions == 5:
            from .qmlp import MLPFast
            self.fast = MLPFast(self.online, self.device, x3=precision != "bf16")
            self.fast_t = MLPFast(self.target, self.device, x3=precision != "bf16")
        self.drop_stream = 0
        # x3 MLP: the TD step inside the backward, the norm partials out of its reductions, clip +
        # Adam + operand repack in one launch (fused_opt = False: the separate td_loss / backward /
        # sumsq / clip_adam / pack3 launches -- tests compare the two)
        self.fused_opt = self.fast is not None and self.fast.x3
        if self.fused_opt:
            assert self.online.numel == int(lib().evx_qmlp_nparams()), "MLP parameter count"
        self._ss = torch.zeros(1024, dtype=torch.float32, device=self.device)
        self._ss_fresh = False

    # ------------------------------------------------------------ dropout
    def dropout_mask(self, B, tag="m"):
        m = self.net.ws.get("mask_" + tag, (B, self.hidden), torch.uint8, self.device)
        check(lib().evx_dropout_mask(_p(m), m.numel(), DROPOUT_P, self.seed, self.rng_offset, _stream()),
              "dropout_mask")
        self.rng_offset += (m.numel() + 3) // 4
        return m

    def q_values(self, x, train=True, mask=None, target=False, tag: str = "act"):
        """tag names this call's scratch (activations, split-K partials, packed weights, dropout
        mask): forwards that may run concurrently on different streams need different tags."""
        B = x.shape[0]
        if mask is None and train:
            mask = self.dropout_mask(B, tag)
        net = self.tnet if target else self.net
        return net.forward(x, mask if train else None, save=False, tag=tag + "_")

    @property
    def _delta(self) -> float:
        """The kernels' huber_delta: 0 selects the squared error."""
        return self.huber_delta if self.loss_kind == "huber" else 0.0

    def _td_loss(self, Q, Qt, a, r, done, B, weights, dQ, td_abs, tw, sel, gamma_row=None):
        """The TD launch of the separate chain: today's entry with the options off."""
        L = lib()
        if gamma_row is not None and (gamma_row.dtype != torch.float32 or gamma_row.numel() < B):
            raise ValueError(f"gamma_row must be a float32 tensor of at least B = {B} elements")
        if sel is None and not self._delta and gamma_row is None:
            check(L.evx_td_loss_w(_p(Q), _p(Qt), self.actions, _p(a), _p(r), _p(done), self.gamma, B, _p(weights),
                                  _p(dQ), _p(self.loss), _p(td_abs), _p(tw), tw.numel(), _stream()), "td_loss")
            return
        o = td_opts(sel, self._delta, gamma_row)
        check(L.evx_td_loss_opt(_p(Q), _p(Qt), self.actions, _p(a), _p(r), _p(done), self.gamma, B, 1, _p(weights),
                                _p(dQ), _p(self.loss), _p(td_abs), None, 0, _p(tw), tw.numel(), C.byref(o),
                                _stream()), "td_loss_opt")

    def learn(self, s, a, r, done, s2, mask_online=None, mask_target=None, weights=None, td_abs=None,
              mask_select=None, gamma_row=None):
        """One DQNAgent.learn step on device tensors; returns the loss tensor (no host sync).
        weights / td_abs: prioritized replay's importance weights in, |TD error| out.
        mask_select: double_q's selection forward's keep mask (as mask_online / mask_target).
        gamma_row: device f32 [B], the discount per row in place of gamma (n-step rows from
        Replay.nstep: r the n-step return, s2 / done the chain's last slot's)."""
        B = s.shape[0]
        if mask_online is None:
            mask_online = self.dropout_mask(B, "on")
        if mask_target is None:
            mask_target = self.dropout_mask(B, "tg")
        sel = None
        if self.double_q:  # the online net's greedy action at s' (train mode, as every forward of learn)
            Qs = self.q_values(s2, train=True, mask=mask_select, target=False, tag="sel")
            sel = self.net.ws.get("sel", (B,), torch.int32, self.device)
            check(lib().evx_act(_p(Qs), B, self.actions, 0.0, 0, 0, _p(sel), _stream()), "act (selection)")
            self.last_sel = sel
        Q = self.net.forward(s, mask_online, save=True)
        Qt = self.tnet.forward(s2, mask_target, save=False, tag="t_")
        dQ = self.net.ws.get("dq", (B, self.actions), torch.float32, self.device)
        tw = td_workspace(self.net.ws, B, 1, self.device)
        self._td_loss(Q, Qt, a, r, done, B, weights, dQ, td_abs, tw, sel, gamma_row)
        if self.stats is not None:
            self.stat_batch = (Q, Qt, a, r, done, sel, gamma_row, B)
        self.net.backward(dQ, self.grads)
        if self.grad_hook is not None:
            self.grad_hook(self.grads.flat)
        self.step_optimizer()
        return self.loss

    def _pair_args(self, lay_c, s_obs, s2_obs, B, mask_online, mask_target, drop_row0):
        """The arguments of learn_obs's forward pair (MLPFast.forward_pair / forward_pair_plan): the
        online net saves X, H1, H2 and Q in the workspace, the target Q; dropout on the current stream
        and the next. drop_row0 (even): the dropout hash rows start there (evacx.qgroup keys net g's
        batch rows g * B + i)."""
        from .qmlp import HID, HID2
        f = self.fast

        def buf(name, per_row, dt):
            return self.net.ws.get(name, (B * per_row,), dt, self.device)
        out0 = dict(h1=buf("fh1", f.planes * HID, torch.int16), x=buf("fx", f.kx, torch.int16),
                    h2=buf("fh2", HID2, torch.float32), q=buf("fq", self.actions, torch.float32))
        out1 = dict(h1=buf("fh1t", f.planes * HID, torch.int16), q=buf("fqt", self.actions, torch.float32))
        d_on = (self.seed, self.drop_stream, DROPOUT_P, mask_online, drop_row0)
        d_tg = (self.seed, self.drop_stream + 1, DROPOUT_P, mask_target, drop_row0)
        return (lay_c, B, f, s_obs, d_on, out0, self.fast_t, s2_obs, d_tg, out1), out0, out1

    def learn_plan(self, lay_c, s_obs, s2_obs, B, mask_online=None, mask_target=None, drop_row0: int = 0):
        """What learn_obs's forward pair launches with these arguments (MLPFast.forward_pair_plan: the
        launcher's own plan, nothing launched; the dropout stream, which learn_obs advances first,
        does not bear on the plan)."""
        pair, _, _ = self._pair_args(lay_c, s_obs, s2_obs, B, mask_online, mask_target, drop_row0)
        return type(self.fast).forward_pair_plan(*pair)

    def learn_obs(self, lay_c, s_obs, a, r, done, s2_obs, B, update: bool = True, weights=None, td_abs=None,
                  mask_online=None, mask_target=None, drop_row0: int = 0, mask_select=None, gamma_row=None):
        """DQNAgent.learn on compact observations with the fused kernels (x3 = f32-accurate,
        or bf16): online forward (saves X, H1, H2), target forward, TD loss, backward,
        clip+Adam. update=False stops after the gradients (the caller runs step_optimizer
        later). mask_online / mask_target: explicit uint8 [B][512] dropout keep masks (tests:
        the reference's captured torch masks) in place of the hash. double_q: one more forward of
        the online net on s2 (the fused act kernel, actions only) on dropout stream drop_stream + 2
        (mask_select: its explicit mask) leaves the bootstrap actions in last_sel. gamma_row: as
        learn's."""
        from .qmlp import HID, HID2, act_ws_ints
        if gamma_row is not None and (gamma_row.dtype != torch.float32 or gamma_row.numel() < B):
            raise ValueError(f"gamma_row must be a float32 tensor of at least B = {B} elements")
        for name, t in (("s_obs", s_obs), ("s2_obs", s2_obs)):  # evx_obs rows are 8 words
            if t.numel() < B * 8:
                raise ValueError(f"learn_obs: {name} holds {t.numel() // 8} observations, B = {B}")
        ws, dev = self.net.ws, self.device
        pl = self.fast.planes

        def buf(name, per_row, dt):
            return ws.get(name, (B * per_row,), dt, dev)
        dQ = buf("fdq", self.actions, torch.float32).view(B, self.actions)
        dz2 = buf("fdz2", pl * HID2, torch.int16)
        dz1 = buf("fdz1", pl * HID, torch.int16)
        self.drop_stream += 3 if self.double_q else 2
        pair, on, tg = self._pair_args(lay_c, s_obs, s2_obs, B, mask_online, mask_target, drop_row0)
        X, H1 = on["x"], on["h1"]
        H2, Q, Qt = on["h2"].view(B, HID2), on["q"].view(B, self.actions), tg["q"].view(B, self.actions)
        sel = None
        if self.double_q:
            # the learner's own buffers: in the lagged schedule this runs on the learn stream beside the
            # trainer's act on the main stream (the act's workspace is zeroed once; every act resets it)
            sel = buf("fsel", 1, torch.int32)
            sws = self._sel_ws.get(B)
            if sws is None:
                sws = self._sel_ws[B] = torch.zeros(act_ws_ints(B), dtype=torch.int32, device=dev)
            self.fast.act(lay_c, s2_obs, B, drop=(self.seed, self.drop_stream + 2, DROPOUT_P, mask_select, drop_row0),
                          actions=sel, epsilon=0.0, ws=sws)
            self.last_sel = sel
        if self.stats is not None:
            self.stat_batch = (Q, Qt, a, r, done, sel, gamma_row, B)
        type(self.fast).forward_pair(*pair)
        if self.fused_opt:
            # the TD step inside the backward's first kernel, the gradients overwritten by its ordered
            # reductions, which also leave the norm partials unless an all-reduce will change the gradients
            self.fast.td_backward(B, Q, Qt, a, r, done, self.gamma, self.loss, X, H1, H2, DROPOUT_P, dz2, dz1,
                                  self.grads, weights=weights, td_abs=td_abs,
                                  ss=self._ss if self.grad_hook is None else None, sel=sel, huber_delta=self._delta,
                                  gamma_row=gamma_row)
            self._ss_fresh = self.grad_hook is None
        else:
            tw = td_workspace(ws, B, 1, dev)
            self._td_loss(Q, Qt, a, r, done, B, weights, dQ, td_abs, tw, sel, gamma_row)
            self.fast.backward(B, dQ, X, H1, H2, DROPOUT_P, dz2, dz1, self.grads)
        if self.grad_hook is not None:
            self.grad_hook(self.grads.flat)
        if update:
            self.step_optimizer()
        return self.loss

    def step_optimizer(self):
        L = lib()
        n = self.online.numel
        if self.fused_opt:  # clip + Adam + x3 repack in one launch from the norm partials
            if not self._ss_fresh:
                self.fast.sumsq_parts(self.grads.flat, self._ss)
            self._ss_fresh = False
            self.adam_step += 1
            h = evx_adam(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=0.0,
                         step=self.adam_step)
            self.fast.adam_step(self.online.flat, self.grads.flat, self.m, self.v, float(self.max_norm or 0.0), h,
                                self._ss, self.norm)
            if self.stats is not None:
                self._stats_update()
            return
        check(L.evx_sumsq_norm(_p(self.grads.flat), n, _p(self.scratch), self.scratch.numel(), _p(self.norm),
                               _stream()), "sumsq")
        self.adam_step += 1
        h = evx_adam(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=0.0,
                     step=self.adam_step)
        check(L.evx_clip_adam(_p(self.online.flat), _p(self.grads.flat), _p(self.m), _p(self.v), n,
                              _p(self.norm) if self.max_norm else None, float(self.max_norm or 0.0), C.byref(h),
                              _stream()), "clip_adam")
        if self.fast is not None:
            self.fast.repack()  # bf16 copies follow the fp32 master parameters
        if self.stats is not None:
            self._stats_update()

    def _stats_update(self):
        """The learn step's batch into the statistics, after Adam has written norm: the buffers the
        step used are the learner's own until the next learn on this stream."""
        if self.stat_batch is None:
            return
        Q, Qt, a, r, done, sel, gamma_row, B = self.stat_batch
        self.stats.update(Q, Qt, a[:B], r[:B], done[:B], self.gamma, B, sel=sel,
                          gamma_row=None if gamma_row is None else gamma_row[:B], loss=self.loss, norm=self.norm,
                          max_norm=float(self.max_norm or 0.0))

    def m_view(self, name: str) -> torch.Tensor:
        """Adam first moment of one parameter (torch's optimizer.state[p]["exp_avg"])."""
        return FlatParams(self.shapes, self.device, data=self.m)[name]

    def v_view(self, name: str) -> torch.Tensor:
        """Adam second moment of one parameter (torch's optimizer.state[p]["exp_avg_sq"])."""
        return FlatParams(self.shapes, self.device, data=self.v)[name]

    def sync_target(self):
        """DQNAgent.update_target_network (agents/dqn_agent.py:170-172)."""
        self.target.flat.copy_(self.online.flat)
        if self.fast_t is not None:
            self.fast_t.repack()

    def soft_update(self):
        """Polyak target update: target = target_tau * online + (1 - target_tau) * target. x3 MLP:
        the blend and the target's operand repack in one launch (then its act table, if attached);
        otherwise the blend on the flat buffers (bf16 MLP: then the repack)."""
        if self.fast_t is not None and self.fast_t.x3:
            self.fast_t.polyak_step(self.online.flat, self.target.flat, self.target_tau)
            return
        t, omt = polyak_coeffs(self.target_tau)
        check(lib().evx_polyak(_p(self.online.flat), _p(self.target.flat), self.target.numel, t, omt, _stream()),
              "polyak")
        if self.fast_t is not None:
            self.fast_t.repack()

    def weights_written(self, target: bool = False):
        """Call after writing a network's fp32 parameters from outside the learner (a
        load_state_dict, a broadcast from another rank): the fused kernels read operand copies
        (bf16 hi / lo tiles) and, once attach_static ran, a per-centre act table of fc1 --
        the learner's online forward reads that table too -- and those are rebuilt only
        here, in sync_target and in the optimizer step."""
        fast = self.fast_t if target else self.fast
        if fast is not None:
            fast.repack()
