"""Terminal health on the device (csrc/health.hip, ``evx_health_*`` in include/evacx.h).

The reference's strategy comparison prints ``EvacuationEnv.get_performance_metrics()`` per
episode (envs/evacuation_env.py:290-309): ``avg_health`` = np.mean of the healths of the
persons that are not dead, ``min_health`` = their min (100 with none). ``HealthStats`` takes
the same numbers from a VecEnv's ``pk`` / ``health`` where ``done`` is set -- after the step and
before the reset, so the envs are stepped with ``auto_reset=False`` and reset with the device
mask afterwards -- one launch per step and no host sync. ``avg_health`` equals np.mean bit for
bit (numpy's summation order is stated in include/evacx.h).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from ._envstats import EnvSlice, check_rows, host_rows, need
from ._lib import HEALTH_MAX_P as MAX_P, HEALTH_ROW_WORDS as ROW_WORDS
from ._lib import check, evx_health, lib
from .env import _ptr, _stream

_I64 = ("n_total", "w_n", "w_has", "w_alive")
_F64 = ("w_avg", "w_min", "w_lo", "last_avg", "last_min")
_I32 = ("last_alive",)
_TAB = ("tab_avg", "tab_min", "tab_alive")
# the loader's earlier name here, kept for callers written against them
hlib = lib


def _row_dict(irow, frow) -> dict:
    n, has = int(irow[0]), int(irow[1])
    d = dict(episodes=n, health_episodes=has, avg_health=None, min_health_mean=None, min_health=None,
             alive_mean=None, alive_sum=int(irow[2]), avg_health_sum=float(frow[3]), min_health_sum=float(frow[4]))
    if has > 0:
        d["avg_health"] = d["avg_health_sum"] / has
    if n > 0:
        d.update(min_health_mean=d["min_health_sum"] / n, min_health=float(frow[5]), alive_mean=d["alive_sum"] / n)
    return d


class _Slice(EnvSlice):
    """``n`` envs of a HealthStats from env ``lo``."""
    _desc, _per_env, _tables, _fixed = evx_health, _I64 + _F64 + _I32, _TAB, {"tab_slots": "record"}

    def update(self, env_or_tensors, done: torch.Tensor):
        """Fold the finished episodes of these envs: ``env_or_tensors`` is a VecEnv (its ``pk`` and
        ``health``) or a pair (pk int32 [E, P], health float64 [E, P]) as the step left them, ``done``
        the step's uint8 flags. One launch on the current stream; envs with done == 0 are untouched."""
        if isinstance(env_or_tensors, (tuple, list)):
            pk, health = env_or_tensors
        else:
            pk, health = env_or_tensors.pk, env_or_tensors.health
        dev, P = self.owner.device, self.owner.P
        need("pk", pk, self.E * P, torch.int32, dev)
        need("health", health, self.E * P, torch.float64, dev)
        need("done", done, self.E, torch.uint8, dev)
        check(lib().evx_health_update(C.byref(self.c), pk.data_ptr(), health.data_ptr(), P, done.data_ptr(),
                                      self.owner.cap, _stream()), "health_update")


class HealthStats(_Slice):
    """Per-env terminal health of E envs of P people each; the arguments are EpisodeStats's.

    Public per-env tensors: the window ``w_n``, ``w_has`` (episodes with somebody alive),
    ``w_alive``, ``w_avg``, ``w_min`` (sums), ``w_lo`` (smallest min_health); the last finished
    episode ``last_avg``, ``last_min``, ``last_alive``; the lifetime count ``n_total``; with
    record = K the table ``tab_avg``, ``tab_min``, ``tab_alive`` [E, K]."""
    _part = _Slice

    def __init__(self, E: int, device, P: int, layout_idx: Optional[torch.Tensor] = None, n_layouts: int = 1,
                 cap: int = 0, record: int = 0):
        E, P, n_layouts, cap, record = int(E), int(P), int(n_layouts), int(cap), int(record)
        if E < 1 or not 1 <= P <= MAX_P:
            raise ValueError(f"HealthStats: E must be >= 1 and P 1..{MAX_P}, not {E}, {P}")
        if cap < 0 or record < 0:
            raise ValueError("HealthStats: cap and record must be >= 0")
        device = check_rows("HealthStats", E, n_layouts, layout_idx, device)
        self.P, self.n_layouts, self.cap, self.record = P, n_layouts, cap, record
        self.layout_idx = layout_idx
        for name in _I64:
            setattr(self, name, torch.zeros(E, dtype=torch.int64, device=device))
        for name in _F64:
            setattr(self, name, torch.zeros(E, dtype=torch.float64, device=device))
        for name in _I32:
            setattr(self, name, torch.zeros(E, dtype=torch.int32, device=device))
        if record:
            self.tab_avg = torch.zeros(E, record, dtype=torch.float64, device=device)
            self.tab_min = torch.zeros(E, record, dtype=torch.float64, device=device)
            self.tab_alive = torch.zeros(E, record, dtype=torch.int32, device=device)
        self.device = self.w_avg.device  # with its index
        self.rows = torch.zeros((n_layouts + 1) * ROW_WORDS, dtype=torch.int64, device=device)
        super().__init__(self, 0, E)
        check(lib().evx_health_init(C.byref(self.c), _stream()), "health_init")

    def summary(self, clear: bool = True) -> dict:
        """Reduce the window over envs (one launch, plus one that empties the window when
        ``clear``), copy the rows to the host (this waits for the current stream) and return the
        "all" row: ``episodes``, ``health_episodes`` (the ones with somebody alive), ``avg_health``
        (mean of avg_health over those, None if none), ``min_health_mean``, ``min_health`` (the
        smallest), ``alive_mean`` (None with no episode), the raw sums, and ``per_layout``."""
        check(lib().evx_health_reduce(C.byref(self.c), _ptr(self.layout_idx), self.n_layouts, self.rows.data_ptr(),
                                      int(bool(clear)), _stream()), "health_reduce")
        irows, frows = host_rows(self.rows, self.n_layouts + 1, ROW_WORDS)
        out = _row_dict(irows[-1], frows[-1])
        out["per_layout"] = [_row_dict(irows[l], frows[l]) for l in range(self.n_layouts)]
        return out


__all__ = ["HealthStats", "evx_health", "MAX_P"]
