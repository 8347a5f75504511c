"""Evacuation timelines and tracked persons on the device (csrc/timeline.hip, ``evx_timeline_*``
in include/evacx.h).

The reference judges a policy with one recorded episode (``DQNTrainingVisualizer``,
utils/visualization.py): evacuated / dead / remaining / ``avg_health`` after every step, the
evacuation-time and death-time distributions from the per-step count deltas, and some selected
persons step by step. ``Timeline`` keeps the same over every episode of every env: per layout row
and episode step the events and the health are added up on the device, one call per step and no
host sync; ``curves()`` copies the tables back and turns them into per-step curves. Everything
added across envs is an integer (health in fixed point at 2^-20), so the numbers do not depend on
the order of the adds.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from ._envstats import check_rows, need
from ._lib import HEALTH_MAX_P as MAX_P
from ._lib import check, evx_timeline, lib
from .env import _ptr, _stream

TIME_PER_STEP = 0.5   # envs/evacuation_env.py:27
Q_ONE = float(1 << 20)  # health_q's unit is 2^-20
MAX_PERSON_STEPS = 1 << 36  # episodes * P a slot may add up: 2^36 * 128 * 2^20 = 2^63
SLOT_FIELDS = ("evac", "dead", "ended", "seen", "alive", "health_q")
SAFE_BIT, DEAD_BIT = 1 << 24, 1 << 25  # pk


def _row_curves(slots: dict, late, P: int) -> dict:
    """The curves of one row: ``slots`` its six [T] int64 arrays, ``late`` its four counters."""
    evac, dead, ended, seen = (np.asarray(slots[k], np.int64) for k in ("evac", "dead", "ended", "seen"))
    alive, hq = np.asarray(slots["alive"], np.int64), np.asarray(slots["health_q"], np.int64)
    episodes = int(seen[0]) if len(seen) else 0  # every recorded episode passes slot 0
    with np.errstate(all="ignore"):
        n = np.float64(episodes) if episodes else np.float64("nan")
        evac_mean = np.cumsum(evac) / n
        dead_mean = np.cumsum(dead) / n
        health = np.where(alive > 0, hq / Q_ONE / np.where(alive > 0, alive, 1), np.nan)
    return dict(episodes=episodes, new_evacuated=evac, new_dead=dead, ended=ended, running=seen, alive=alive,
                evacuated_mean=evac_mean, dead_mean=dead_mean, remaining_mean=P - evac_mean - dead_mean,
                avg_health=health, late=np.asarray(late, np.int64))


def build_curves(slots: dict, late, bad_health: int, P: int, trace: Optional[dict] = None) -> dict:
    """``Timeline.curves()`` from host arrays, no device: ``slots`` the six [n_rows, T] int64 tables
    (``evac``, ``dead``, ``ended``, ``seen``, ``alive``, ``health_q``), ``late`` [n_rows, 4],
    ``trace`` = dict(env, person, pk [T + 1, n], health [T + 1, n], len [n]) or None.

    Returns ``step`` (1..T), ``time_s`` (step * 0.5) and, over all rows summed (integer sums,
    exact): ``episodes``; ``new_evacuated``, ``new_dead`` (the reference's per-step deltas: the
    evacuation-time and death-time distributions), ``ended``, ``running`` (episodes recorded at
    the step), ``alive``; ``evacuated_mean`` / ``dead_mean`` = the cumulative events / episodes (an
    ended episode carries its terminal counts on, so the curve is over all episodes),
    ``remaining_mean`` = P - both; ``avg_health`` = health_q / 2^20 / alive (NaN where nobody is
    counted); ``late`` (evac, dead, ended, steps beyond T); ``bad_health``; ``per_layout`` the
    same per row; and with a trace ``tracked``."""
    tabs = {k: np.asarray(slots[k], np.int64) for k in SLOT_FIELDS}
    late = np.asarray(late, np.int64).reshape(-1, 4)
    n_rows, T = tabs["seen"].shape
    out = _row_curves({k: v.sum(axis=0) for k, v in tabs.items()}, late.sum(axis=0), P)
    step = np.arange(1, T + 1, dtype=np.int64)
    out.update(step=step, time_s=step * TIME_PER_STEP, bad_health=int(bad_health),
               per_layout=[_row_curves({k: v[r] for k, v in tabs.items()}, late[r], P) for r in range(n_rows)])
    if trace is not None:
        out["tracked"] = decode_trace(trace)
    return out


def _first_slot(bit: np.ndarray, length: np.ndarray) -> np.ndarray:
    """Per column the first slot < length whose bit is set, -1 without one."""
    on = bit & (np.arange(bit.shape[0])[:, None] < length[None, :])
    return np.where(on.any(axis=0), on.argmax(axis=0), -1).astype(np.int64)


def decode_trace(trace: dict) -> dict:
    """The tracked persons' trace in plain terms: ``x``, ``y``, ``safe``, ``dead``, ``health``
    [T + 1, n] (slot 0 after the reset, slot t after step t; slots >= ``len`` were not written),
    ``evac_step`` / ``death_step`` the first slot that carries the bit (-1: never)."""
    pk = np.asarray(trace["pk"]).view(np.uint32)
    length = np.asarray(trace["len"], np.int64)
    safe, dead = (pk & SAFE_BIT) != 0, (pk & DEAD_BIT) != 0
    return dict(env=np.asarray(trace["env"], np.int64), person=np.asarray(trace["person"], np.int64),
                x=(pk & 0xFFF).astype(np.int32), y=((pk >> 12) & 0xFFF).astype(np.int32), safe=safe, dead=dead,
                health=np.asarray(trace["health"], np.float64), len=length,
                evac_step=_first_slot(safe, length), death_step=_first_slot(dead, length))


class Timeline:
    """Per-step evacuation curves of E envs of P people each over T steps per episode.

    layout_idx / n_layouts / cap are EpisodeStats's: one row per layout, and with cap > 0 only the
    first ``cap`` episodes of every env are recorded. track = (env_ids, person_ids), or an int n
    for the first n persons of env 0 (the reference picks 20): those persons' ``pk`` and health are
    kept for every step of their env's first episode. E * max(cap, 1) * P beyond 2^36 is refused:
    below it a slot's fixed-point health sum cannot overflow.

    Public tensors: per env ``t``, ``p_evac``, ``p_dead``, ``n_total``; the tables ``evac``,
    ``dead``, ``ended``, ``seen``, ``alive``, ``health_q`` [n_layouts, T]; ``late`` [n_layouts, 4];
    ``bad_health`` [1]; ``trk_env``, ``trk_person``, ``trk_len`` [n], ``trk_pk``, ``trk_health``
    [T + 1, n]."""

    def __init__(self, E: int, device, P: int, T: int = 1200, layout_idx: Optional[torch.Tensor] = None,
                 n_layouts: int = 1, cap: int = 0, track=None):
        E, P, T, n_layouts, cap = int(E), int(P), int(T), int(n_layouts), int(cap)
        if E < 1 or T < 1 or not 1 <= P <= MAX_P:
            raise ValueError(f"Timeline: E and T must be >= 1 and P 1..{MAX_P}, not {E}, {T}, {P}")
        if cap < 0:
            raise ValueError("Timeline: cap must be >= 0")
        if E * max(cap, 1) * P >= MAX_PERSON_STEPS:
            raise ValueError(f"Timeline: E * cap * P = {E * max(cap, 1) * P} is not below 2^36, a slot's health "
                             "sum could overflow")
        env_ids, person_ids = self._track_ids(track, E, P)
        device = check_rows("Timeline", E, n_layouts, layout_idx, device, where="the timeline is")
        self.E, self.P, self.T, self.n_layouts, self.cap = E, P, T, n_layouts, cap
        self.layout_idx, self.n_trk = layout_idx, len(env_ids)
        i32, i64 = dict(dtype=torch.int32, device=device), dict(dtype=torch.int64, device=device)
        for name in ("t", "p_evac", "p_dead"):
            setattr(self, name, torch.zeros(E, **i32))
        self.n_total = torch.zeros(E, **i64)
        for name in SLOT_FIELDS:
            setattr(self, name, torch.zeros(n_layouts, T, **i64))
        self.late = torch.zeros(n_layouts, 4, **i64)
        self.bad_health = torch.zeros(1, **i64)
        self.device = self.t.device  # with its index
        names = ["t", "p_evac", "p_dead", "n_total", *SLOT_FIELDS, "late", "bad_health"]
        if self.n_trk:
            n = self.n_trk
            self.trk_env = torch.tensor(env_ids, **i32)
            self.trk_person = torch.tensor(person_ids, **i32)
            self.trk_pk = torch.zeros(T + 1, n, **i32)
            self.trk_health = torch.zeros(T + 1, n, dtype=torch.float64, device=device)
            self.trk_len = torch.zeros(n, **i32)
            names += ["trk_env", "trk_person", "trk_pk", "trk_health", "trk_len"]
        self.c = evx_timeline(E=E, T=T, n_rows=n_layouts, n_trk=self.n_trk)
        for name in names:
            setattr(self.c, name, _ptr(getattr(self, name)))
        check(lib().evx_timeline_init(C.byref(self.c), _stream()), "timeline_init")

    @staticmethod
    def _track_ids(track, E: int, P: int):
        if track is None:
            return [], []
        if isinstance(track, bool):
            raise ValueError("track: a person count or (env_ids, person_ids) is needed")
        if isinstance(track, int):
            if not 0 <= track <= P:
                raise ValueError(f"track: 0..{P} persons of env 0 can be tracked, not {track}")
            return [0] * track, list(range(track))
        env_ids, person_ids = ([int(v) for v in ids] for ids in track)
        if len(env_ids) != len(person_ids):
            raise ValueError("track: env_ids and person_ids differ in length")
        if any(not 0 <= e < E for e in env_ids) or any(not 0 <= p < P for p in person_ids):
            raise ValueError(f"track: an env is not within 0..{E - 1} or a person not within 0..{P - 1}")
        return env_ids, person_ids

    def _state(self, env_or_tensors):
        if isinstance(env_or_tensors, (tuple, list)):
            pk, health = env_or_tensors
        else:
            pk, health = env_or_tensors.pk, env_or_tensors.health
        need("pk", pk, self.E * self.P, torch.int32, self.device)
        need("health", health, self.E * self.P, torch.float64, self.device)
        return pk, health

    def update(self, env, done: torch.Tensor, counts: torch.Tensor):
        """Count one step of every env: ``env`` is a VecEnv (its ``pk`` and ``health``) or a pair
        (pk int32 [E, P], health float64 [E, P]) as the step left them and before any reset, or
        None where the resets are fused into the step (``alive`` / ``health_q`` then stay; not with
        tracked persons); ``done`` / ``counts`` the step's outputs. One launch on the current
        stream, and one before it with tracked persons."""
        pk, health = (None, None) if env is None else self._state(env)
        need("done", done, self.E, torch.uint8, self.device)
        need("counts", counts, 2 * self.E, torch.int32, self.device)
        check(lib().evx_timeline_update(C.byref(self.c), counts.data_ptr(), done.data_ptr(), _ptr(self.layout_idx),
                                        _ptr(pk), _ptr(health), self.P, self.cap, _stream()), "timeline_update")

    def trace0(self, env):
        """Slot 0 of the tracked persons: call after the first reset. One launch, none without a trace."""
        pk, health = self._state(env)
        check(lib().evx_timeline_trace0(C.byref(self.c), pk.data_ptr(), health.data_ptr(), self.P, _stream()),
              "timeline_trace0")

    def curves(self) -> dict:
        """Copy the tables to the host (this waits for the current stream) and return
        ``build_curves`` of them: plain numpy."""
        slots = {k: getattr(self, k).cpu().numpy() for k in SLOT_FIELDS}
        trace = None
        if self.n_trk:
            trace = dict(env=self.trk_env.cpu().numpy(), person=self.trk_person.cpu().numpy(),
                         pk=self.trk_pk.cpu().numpy(), health=self.trk_health.cpu().numpy(),
                         len=self.trk_len.cpu().numpy())
        return build_curves(slots, self.late.cpu().numpy(), int(self.bad_health.item()), self.P, trace)


__all__ = ["Timeline", "build_curves", "decode_trace", "evx_timeline"]
