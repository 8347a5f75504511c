"""Episode statistics on the device (csrc/episode.hip, ``evx_episode_*`` in include/evacx.h).

The reference's training loop logs each episode's total reward, ``evacuation_rate`` and
``death_rate`` on the host (runners/train_dqn.py:129-161). The vectorised envs reset inside
the step launch and overwrite ``reward``, ``done`` and ``counts`` one step later, so
``EpisodeStats`` folds them per env on the device, one launch per step and no host sync;
``summary()`` reduces the window over envs (one fixed summation order) and copies a few
hundred bytes back.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from ._envstats import EnvSlice, as_mask, check_rows, host_rows, need
from ._lib import EPISODE_REDUCE_SPAN as REDUCE_SPAN, EPISODE_ROW_WORDS as ROW_WORDS  # noqa: F401
from ._lib import check, evx_episodes, lib
from .env import _ptr, _stream

_I64 = ("w_n", "w_len", "w_evac", "w_dead", "n_total")
_F64 = ("ret", "w_ret", "w_ret2", "w_min", "w_max", "last_ret")
_I32 = ("len", "last_len", "last_evac", "last_dead")
_TAB = ("tab_ret", "tab_len", "tab_evac", "tab_dead")
# the loader's earlier name here, kept for callers written against them
elib = lib


def _row_dict(irow, frow, P: int) -> dict:
    n = int(irow[0])
    d = dict(episodes=n, return_min=None, return_max=None, return_mean=None, return_std=None, length_mean=None,
             evac_rate=None, death_rate=None, remaining=int(irow[8]), no_episode=int(irow[9]),
             length_sum=int(irow[1]), evacuated=int(irow[2]), dead=int(irow[3]),
             return_sum=float(frow[4]), return_sq_sum=float(frow[5]))
    if n > 0:
        mean = d["return_sum"] / n
        d.update(return_mean=mean, return_std=math.sqrt(max(d["return_sq_sum"] / n - mean * mean, 0.0)),
                 return_min=float(frow[6]), return_max=float(frow[7]), length_mean=d["length_sum"] / n,
                 evac_rate=d["evacuated"] / (n * P), death_rate=d["dead"] / (n * P))
    return d


class _Slice(EnvSlice):
    """``n`` envs of an EpisodeStats from env ``lo`` (a VecEnv.split part's own envs)."""
    _desc, _per_env, _tables, _fixed = evx_episodes, _I64 + _F64 + _I32, _TAB, {"tab_slots": "record"}

    def update(self, reward: torch.Tensor, done: torch.Tensor, counts: torch.Tensor):
        """Fold one step's outputs of these envs (VecEnv.reward / done / counts), one launch on
        the current stream."""
        dev = self.owner.device
        need("reward", reward, self.E, torch.float64, dev)
        need("done", done, self.E, torch.uint8, dev)
        need("counts", counts, 2 * self.E, torch.int32, dev)
        check(lib().evx_episode_update(C.byref(self.c), reward.data_ptr(), done.data_ptr(), counts.data_ptr(),
                                       self.owner.cap, _stream()), "episode_update")

    def discard(self, mask: Optional[torch.Tensor] = None):
        """Drop the episode in progress of the masked envs (None: all): for envs reset from
        outside the step. One launch on the current stream."""
        m = as_mask(mask, self.E, self.owner.device)
        check(lib().evx_episode_discard(C.byref(self.c), _ptr(m), _stream()), "episode_discard")


class EpisodeStats(_Slice):
    """Per-env episode statistics of E envs of P people each.

    layout_idx / n_layouts: each env's layout (VecEnv.layout_idx of a LayoutSet) for the
    per-layout rows of ``summary``. cap > 0: only the first ``cap`` episodes of every env
    enter the window (an evaluation over exactly E * cap episodes). record = K > 0: the
    first K episodes of every env are also kept one by one (``tab_ret`` ... [E, K]).

    Public per-env tensors: the episode in progress ``ret``, ``len``; the window ``w_n``,
    ``w_len``, ``w_evac``, ``w_dead``, ``w_ret``, ``w_ret2``, ``w_min``, ``w_max``; the last
    finished episode ``last_return`` (= ``last_ret``), ``last_len``, ``last_evac``,
    ``last_dead``; the lifetime count ``n_total``."""
    _part = _Slice

    def __init__(self, E: int, device, P: int, layout_idx: Optional[torch.Tensor] = None, n_layouts: int = 1,
                 cap: int = 0, record: int = 0):
        E, P, n_layouts, cap, record = int(E), int(P), int(n_layouts), int(cap), int(record)
        if E < 1 or P < 1:
            raise ValueError(f"EpisodeStats: E and P must be >= 1, not {E}, {P}")
        if cap < 0 or record < 0:
            raise ValueError("EpisodeStats: cap and record must be >= 0")
        device = check_rows("EpisodeStats", E, n_layouts, layout_idx, device)
        self.P, self.n_layouts, self.cap, self.record, self.device = P, n_layouts, cap, record, device
        self.layout_idx = layout_idx
        for name in _I64:
            setattr(self, name, torch.zeros(E, dtype=torch.int64, device=device))
        for name in _F64:
            setattr(self, name, torch.zeros(E, dtype=torch.float64, device=device))
        for name in _I32:
            setattr(self, name, torch.zeros(E, dtype=torch.int32, device=device))
        if record:
            self.tab_ret = torch.zeros(E, record, dtype=torch.float64, device=device)
            for name in _TAB[1:]:
                setattr(self, name, torch.zeros(E, record, dtype=torch.int32, device=device))
        self.device = self.ret.device  # with its index
        self.last_return = self.last_ret
        self.rows = torch.zeros((n_layouts + 1) * ROW_WORDS, dtype=torch.int64, device=device)
        super().__init__(self, 0, E)
        check(lib().evx_episode_init(C.byref(self.c), _stream()), "episode_init")

    def summary(self, clear: bool = True) -> dict:
        """Reduce the window over envs (one launch, plus one that empties the window when
        ``clear``), copy the rows to the host (this waits for the current stream) and return
        the "all" row as a dict, with ``per_layout`` a list of the same dicts. With no episode
        in the window the means and rates are None."""
        check(lib().evx_episode_reduce(C.byref(self.c), _ptr(self.layout_idx), self.n_layouts, self.cap,
                                       self.rows.data_ptr(), int(bool(clear)), _stream()), "episode_reduce")
        irows, frows = host_rows(self.rows, self.n_layouts + 1, ROW_WORDS)
        out = _row_dict(irows[-1], frows[-1], self.P)
        out["per_layout"] = [_row_dict(irows[l], frows[l], self.P) for l in range(self.n_layouts)]
        return out


__all__ = ["EpisodeStats", "evx_episodes", "REDUCE_SPAN"]
