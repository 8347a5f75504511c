"""Learner diagnostics on the device (csrc/lstats.hip, ``evx_lstats_*`` / ``evx_vprobe_*`` in
include/evacx.h).

``LearnStats`` accumulates, per learn step and per net, the Q-values, targets and TD errors of the
sampled batch (sums, extremes, an octave histogram of |TD| for percentiles), the batch's action
histogram and greedy fraction, the loss, the pre-clip gradient norm and how often it was clipped,
and counts of non-finite rows and steps. ``ValueProbe`` keeps, for every episode of every env, the
Q-value the act computed at the episode's first step beside the discounted return the episode then
obtained: the window's mean(Q0 - G) is the over-estimation Double-Q is there to lower.

Both only read (the learner's buffers after its optimizer step, the act's Q output and the env
step's reward / done) and wait for nothing: two launches per learn step, one per env step;
``summary()`` copies a few hundred bytes back at the log interval.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from ._envstats import EnvSlice, as_mask, check_rows, host_rows, need
from ._lib import EPISODE_REDUCE_SPAN as REDUCE_SPAN  # noqa: F401
from ._lib import LSTATS_MAX_A as MAX_A, LSTATS_TD_BUCKETS as TD_BUCKETS, VPROBE_ROW_WORDS as ROW_WORDS
from ._lib import check, evx_lstats, evx_td_opts, evx_vprobe, lib
from .env import _ptr, _stream

_LS_I64 = ("steps", "steps_bad", "rows", "rows_bad", "n_done", "n_greedy", "n_clipped")
_LS_SUM = ("s_q", "s_qmax", "s_y", "s_d", "s_absd", "s_d2", "s_rew", "s_loss", "s_norm")
_LS_EXT = ("max_absd", "max_q", "min_q", "max_loss", "max_norm")
_VP_F64 = ("q0", "g", "disc", "w_q", "w_g", "w_e", "w_e2", "w_q2", "w_g2", "w_qg", "w_emin", "w_emax")
_VP_I64 = ("w_n", "w_bad")


def ws_doubles(B: int, nets: int) -> int:
    """evx_lstats_ws_doubles: the workspace one update of B rows per net needs."""
    return int(lib().evx_lstats_ws_doubles(int(B), int(nets)))


def td_percentile(hist, p: float, td_abs_max: Optional[float]):
    """The upper edge 2^(k - 23) of the first bucket of the |TD| octave histogram whose cumulative
    count reaches p x (its total); the last bucket is open-ended and reports td_abs_max. None for an
    empty histogram."""
    total = sum(int(c) for c in hist)
    if total <= 0:
        return None
    need, cum = p * total, 0
    for k, c in enumerate(hist):
        cum += int(c)
        if cum >= need and cum > 0:
            return td_abs_max if k == len(hist) - 1 else 2.0 ** (k - 23)
    return td_abs_max


def _net_dict(f: dict, A: int) -> dict:
    """One net's (or the total's) window as a dict; f: field -> int / float / list."""
    steps, rows, bad = f["steps"], f["rows"], f["rows_bad"]
    good, gsteps = rows - bad, steps - f["steps_bad"]
    d = dict(steps=steps, rows=rows, rows_bad=bad, steps_bad=f["steps_bad"])
    keys = ("q_mean", "qmax_mean", "target_mean", "td_mean", "td_abs_mean", "reward_mean", "td_rms", "td_abs_max",
            "q_max", "q_min", "td_p50", "td_p90", "td_p99", "greedy_frac", "done_frac", "action_frac", "loss_mean",
            "grad_norm_mean", "loss_max", "grad_norm_max", "clipped_frac")
    d.update({k: None for k in keys})
    if good > 0:
        d.update(q_mean=f["s_q"] / good, qmax_mean=f["s_qmax"] / good, target_mean=f["s_y"] / good,
                 td_mean=f["s_d"] / good, td_abs_mean=f["s_absd"] / good, reward_mean=f["s_rew"] / good,
                 td_rms=math.sqrt(f["s_d2"] / good), td_abs_max=f["max_absd"], q_max=f["max_q"], q_min=f["min_q"],
                 greedy_frac=f["n_greedy"] / good, done_frac=f["n_done"] / good,
                 action_frac=[c / good for c in f["act_hist"][:A]])
        for name, p in (("td_p50", 0.5), ("td_p90", 0.9), ("td_p99", 0.99)):
            d[name] = td_percentile(f["td_hist"], p, f["max_absd"])
    if gsteps > 0:
        d.update(loss_mean=f["s_loss"] / gsteps, grad_norm_mean=f["s_norm"] / gsteps,
                 clipped_frac=f["n_clipped"] / gsteps)
        # a window that was given no loss (norm) keeps the empty extreme
        d["loss_max"] = f["max_loss"] if f["max_loss"] != -math.inf else None
        d["grad_norm_max"] = f["max_norm"] if f["max_norm"] != -math.inf else None
    return d


class LearnStats:
    """The learn-batch statistics of ``nets`` nets with A actions, accumulated on ``device``.

    Public device tensors, per net: the int64 counts ``steps``, ``steps_bad``, ``rows``,
    ``rows_bad``, ``n_done``, ``n_greedy``, ``n_clipped``, ``act_hist`` [nets, 8], ``td_hist``
    [nets, 48]; the float64 sums ``s_q``, ``s_qmax``, ``s_y``, ``s_d``, ``s_absd``, ``s_d2``,
    ``s_rew``, ``s_loss``, ``s_norm``; the extremes ``max_absd``, ``max_q``, ``min_q``,
    ``max_loss``, ``max_norm``."""

    def __init__(self, nets: int, device, A: int = 5):
        nets, A = int(nets), int(A)
        if not 1 <= nets <= 64:
            raise ValueError(f"LearnStats: nets must be 1..64, not {nets}")
        if not 1 <= A <= MAX_A:
            raise ValueError(f"LearnStats: A must be 1..{MAX_A}, not {A}")
        device = torch.device(device)
        self.nets, self.A = nets, A
        for name in _LS_I64:
            setattr(self, name, torch.zeros(nets, dtype=torch.int64, device=device))
        self.act_hist = torch.zeros(nets, MAX_A, dtype=torch.int64, device=device)
        self.td_hist = torch.zeros(nets, TD_BUCKETS, dtype=torch.int64, device=device)
        for name in _LS_SUM + _LS_EXT:
            setattr(self, name, torch.zeros(nets, dtype=torch.float64, device=device))
        self.device = self.steps.device  # with its index
        self.c = evx_lstats(nets=nets, A=A)
        for name in _LS_I64 + ("act_hist", "td_hist") + _LS_SUM + _LS_EXT:
            setattr(self.c, name, getattr(self, name).data_ptr())
        self._ws, self._ws_B = None, 0
        self.clear()

    def clear(self):
        """Empty the window (evx_lstats_init, one launch on the current stream)."""
        check(lib().evx_lstats_init(C.byref(self.c), _stream()), "lstats_init")

    def update(self, Q, Qt, a, r, done, gamma: float, B: int, sel=None, gamma_row=None, loss=None, norm=None,
               max_norm: float = 0.0, d_out=None):
        """Fold one learn step into the window, two launches on the current stream: net g's rows
        are [g B, (g + 1) B) of Q / Qt (float32 [nets * B, A]), a (int32), r (float32), done (uint8),
        sel (int32, the bootstrap actions; None: the target's maximum) and gamma_row (float32, the
        rows' discounts; None: gamma). loss / norm: float32 device scalars per net (what
        step_optimizer leaves); max_norm: the clip threshold (0: none). d_out (float32 [nets * B],
        optional) receives every row's TD error, NaN for a non-finite row."""
        B = int(B)
        if B < 1:
            raise ValueError(f"LearnStats.update: B must be >= 1, not {B}")
        n, dev = self.nets * B, self.device
        need("Q", Q, n * self.A, torch.float32, dev)
        need("Qt", Qt, n * self.A, torch.float32, dev)
        need("a", a, n, torch.int32, dev)
        need("r", r, n, torch.float32, dev)
        need("done", done, n, torch.uint8, dev)
        for name, t, per, dt in (("sel", sel, n, torch.int32), ("gamma_row", gamma_row, n, torch.float32),
                                 ("loss", loss, self.nets, torch.float32), ("norm", norm, self.nets, torch.float32),
                                 ("d_out", d_out, n, torch.float32)):
            if t is not None:
                need(name, t, per, dt, dev)
        if not math.isfinite(gamma):
            raise ValueError(f"LearnStats.update: gamma must be finite, not {gamma}")
        if self._ws is None or self._ws_B < B:  # the block partials' workspace, grown with B
            self._ws = torch.zeros(ws_doubles(B, self.nets), dtype=torch.float64, device=dev)
            self._ws_B = B
        o = evx_td_opts(sel=_ptr(sel), huber_delta=0.0, gamma_row=_ptr(gamma_row))
        check(lib().evx_lstats_update(C.byref(self.c), Q.data_ptr(), Qt.data_ptr(), a.data_ptr(), r.data_ptr(),
                                      done.data_ptr(), float(gamma), B, C.byref(o), _ptr(loss), _ptr(norm),
                                      float(max_norm or 0.0), _ptr(d_out), self._ws.data_ptr(), self._ws.numel(),
                                      _stream()), "lstats_update")

    def fields(self) -> dict:
        """The window copied to the host (this waits for the current stream): field -> list per net."""
        out = {k: getattr(self, k).tolist() for k in _LS_I64 + _LS_SUM + _LS_EXT}
        out["act_hist"] = self.act_hist.tolist()
        out["td_hist"] = self.td_hist.tolist()
        return out

    def summary(self, clear: bool = True) -> dict:
        """The window as a dict (nets == 1), or the total over nets with ``per_net`` a list of the
        nets' dicts. Counts ``steps``, ``rows``, ``rows_bad``, ``steps_bad``; means ``q_mean``,
        ``qmax_mean``, ``target_mean``, ``td_mean``, ``td_abs_mean``, ``reward_mean``, ``loss_mean``,
        ``grad_norm_mean``; ``td_rms``, ``td_abs_max``, ``q_max``, ``q_min``, ``loss_max``,
        ``grad_norm_max``; the percentiles ``td_p50`` / ``td_p90`` / ``td_p99`` (td_percentile);
        ``greedy_frac``, ``done_frac``, ``action_frac`` [A], ``clipped_frac``. The total's ``steps``
        is net 0's (every update steps every net); its sums are added over nets in net order. What
        an empty window cannot give is None. Copies to the host (waits for the current stream);
        clear: then empties the window."""
        f = self.fields()
        if clear:
            self.clear()
        per = [_net_dict({k: v[g] for k, v in f.items()}, self.A) for g in range(self.nets)]
        if self.nets == 1:
            return per[0]
        tot = {}
        for k in _LS_I64 + _LS_SUM:
            s = 0 if k in _LS_I64 else 0.0
            for v in f[k]:
                s = s + v
            tot[k] = s
        tot["act_hist"] = [sum(col) for col in zip(*f["act_hist"])]
        tot["td_hist"] = [sum(col) for col in zip(*f["td_hist"])]
        for k in _LS_EXT:
            tot[k] = min(f[k]) if k == "min_q" else max(f[k])
        out = _net_dict(tot, self.A)
        out["net_steps"] = out["steps"]  # steps summed over nets (steps_bad counts per net too)
        out["steps"] = f["steps"][0]
        out["per_net"] = per
        return out


def probe_stats(n: int, bad: int, open_: int, q: float, g: float, e: float, e2: float, q2: float, g2: float,
                qg: float, emin: float, emax: float) -> dict:
    """One reduced row of the value probe as a dict: ``probes``, ``bad``, ``open``, ``q0_mean``,
    ``return_mean`` (discounted), ``bias`` = mean(Q0 - G), ``rmse``, ``corr`` (Pearson, from the
    sums in float64; None when a variance is 0), ``err_min``, ``err_max``."""
    d = dict(probes=int(n), bad=int(bad), open=int(open_), q0_mean=None, return_mean=None, bias=None, rmse=None,
             corr=None, err_min=None, err_max=None)
    if n > 0:
        d.update(q0_mean=q / n, return_mean=g / n, bias=e / n, rmse=math.sqrt(max(e2 / n, 0.0)), err_min=emin,
                 err_max=emax)
        vq, vg = q2 / n - (q / n) * (q / n), g2 / n - (g / n) * (g / n)
        if vq > 0.0 and vg > 0.0:
            d["corr"] = (qg / n - (q / n) * (g / n)) / math.sqrt(vq * vg)
    return d


class _ProbeSlice(EnvSlice):
    """``n`` envs of a ValueProbe from env ``lo``."""
    _desc, _per_env, _fixed = evx_vprobe, ("open", "len") + _VP_F64 + _VP_I64, {"R": "R", "A": "A"}

    def update(self, Q: torch.Tensor, act: torch.Tensor, reward: torch.Tensor, done: torch.Tensor):
        """One step of these envs, one launch on the current stream: Q (float32 [E * R, A]) and act
        (int32 [E * R]) of the act that chose the step's actions, the step's reward (float64 [E])
        and done (uint8 [E])."""
        o = self.owner
        need("Q", Q, self.E * o.R * o.A, torch.float32, o.device)
        need("act", act, self.E * o.R, torch.int32, o.device)
        need("reward", reward, self.E, torch.float64, o.device)
        need("done", done, self.E, torch.uint8, o.device)
        check(lib().evx_vprobe_update(C.byref(self.c), Q.data_ptr(), act.data_ptr(), reward.data_ptr(),
                                      done.data_ptr(), o.gamma, _stream()), "vprobe_update")

    def discard(self, mask: Optional[torch.Tensor] = None):
        """Close the probes of the masked envs (None: all) without folding them: for envs reset
        from outside the step. One launch on the current stream."""
        m = as_mask(mask, self.E, self.owner.device)
        check(lib().evx_vprobe_discard(C.byref(self.c), _ptr(m), _stream()), "vprobe_discard")


class ValueProbe(_ProbeSlice):
    """The value probe of E envs of R robots: per env the probe in progress (``open``, ``q0``,
    ``g``, ``disc``, ``len``) and the window (``w_n``, ``w_bad``, ``w_q``, ``w_g``, ``w_e``,
    ``w_e2``, ``w_q2``, ``w_g2``, ``w_qg``, ``w_emin``, ``w_emax``), public device tensors [E].
    gamma: the discount of the return (the learner's). layout_idx / n_layouts: as EpisodeStats."""
    _part = _ProbeSlice

    def __init__(self, E: int, R: int, device, gamma: float, layout_idx: Optional[torch.Tensor] = None,
                 n_layouts: int = 1, A: int = 5):
        E, R, A, n_layouts = int(E), int(R), int(A), int(n_layouts)
        if E < 1 or R < 1:
            raise ValueError(f"ValueProbe: E and R must be >= 1, not {E}, {R}")
        if not 1 <= A <= MAX_A:
            raise ValueError(f"ValueProbe: A must be 1..{MAX_A}, not {A}")
        gamma = float(gamma)
        if not (math.isfinite(gamma) and 0.0 <= gamma <= 1.0):
            raise ValueError(f"ValueProbe: gamma must be in [0, 1], not {gamma}")
        device = check_rows("ValueProbe", E, n_layouts, layout_idx, device, where="the probe is")
        self.R, self.A, self.gamma, self.n_layouts, self.layout_idx = R, A, gamma, n_layouts, layout_idx
        self.open = torch.zeros(E, dtype=torch.uint8, device=device)
        self.len = torch.zeros(E, dtype=torch.int32, device=device)
        for name in _VP_F64:
            setattr(self, name, torch.zeros(E, dtype=torch.float64, device=device))
        for name in _VP_I64:
            setattr(self, name, torch.zeros(E, dtype=torch.int64, device=device))
        self.device = self.open.device  # with its index
        self.rows = torch.zeros((n_layouts + 1) * ROW_WORDS, dtype=torch.int64, device=device)
        super().__init__(self, 0, E)
        check(lib().evx_vprobe_init(C.byref(self.c), _stream()), "vprobe_init")

    def reduce(self, clear: bool = False) -> torch.Tensor:
        """evx_vprobe_reduce into ``rows`` (int64 words, [n_layouts + 1, 12]: probes, bad, open, then
        nine float64 bit patterns); returned on the host."""
        check(lib().evx_vprobe_reduce(C.byref(self.c), _ptr(self.layout_idx), self.n_layouts, self.rows.data_ptr(),
                                      int(bool(clear)), _stream()), "vprobe_reduce")
        return self.rows.cpu().view(self.n_layouts + 1, ROW_WORDS)

    def summary(self, clear: bool = True) -> dict:
        """Reduce the window over envs in the fixed order (one launch, plus one that empties the
        window when ``clear``; the probes in progress stay), copy the rows back (waits for the current
        stream) and return the "all" row as probe_stats' dict, with ``per_layout`` a list of the
        same."""
        irows, frows = host_rows(self.reduce(clear), self.n_layouts + 1, ROW_WORDS)
        rows = [probe_stats(*irows[k][:3], *frows[k][3:]) for k in range(self.n_layouts + 1)]
        out = rows[-1]
        out["per_layout"] = rows[:-1]
        return out


__all__ = ["LearnStats", "ValueProbe", "td_percentile", "probe_stats", "ws_doubles", "evx_lstats", "evx_vprobe"]
