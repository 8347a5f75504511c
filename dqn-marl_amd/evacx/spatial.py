"""Spatial maps on the device (csrc/spatial.hip, ``evx_spatial_*`` in include/evacx.h): where an
evacuation happened.

The reference keeps one per-env diagnostic, ``People.thmap`` (envs/people.py), and aggregates
nothing. ``SpatialMaps`` counts, per layout and grid cell and over every counted episode of every
env, the persons that arrived on a cell, stood still on it, left through it (``evac``) or died on
it, and the robots' positions: one call per step between the step and the reset taken apart from
it, no host sync; ``maps()`` copies the counts back and derives occupancy, density, the stall
ratio, the exits' shares and the stall hotspots. Every number is an integer count, so nothing
depends on the order of the adds.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from ._envstats import check_rows, need
from ._lib import HEALTH_MAX_P as MAX_P
from ._lib import SPATIAL, SPATIAL_MAX_GRID, check, evx_spatial, evx_spatial_launch, lib
from .env import _ptr, _stream

MAP_FIELDS = ("arrive", "stall", "evac", "died", "robot")
N_HOTSPOTS = 10

# what SpatialMaps reads of a layout: the padded grid, persons and robots per env
Grid = namedtuple("Grid", ["GX", "GY", "P", "R"])


def _row_maps(counts: dict, steps: int, episodes: int) -> dict:
    """The entry of one row: ``counts`` its five [GX, GY] int64 arrays."""
    out = {k: np.asarray(counts[k], np.int64) for k in MAP_FIELDS}
    GX, GY = out["stall"].shape
    occ = out["arrive"] + out["stall"]
    with np.errstate(all="ignore"):
        density = occ / np.float64(steps) if steps else np.full(occ.shape, np.nan)
        ratio = np.where(occ > 0, out["stall"] / np.where(occ > 0, occ, 1), np.nan)
    evac, stall = out["evac"].reshape(-1), out["stall"].reshape(-1)
    total = int(evac.sum())
    cells = np.nonzero(evac)[0]
    cells = cells[np.lexsort((cells, -evac[cells]))]  # largest count first, ties by cell index
    exit_use = [(int(c) // GY, int(c) % GY, int(evac[c]), int(evac[c]) / total) for c in cells]
    hot = np.lexsort((np.arange(stall.size), -stall))[:N_HOTSPOTS]
    hotspots = [(int(c) // GY, int(c) % GY, int(stall[c])) for c in hot if stall[c] > 0]
    out.update(occupancy=occ, steps=int(steps), episodes=int(episodes), density=density, stall_ratio=ratio,
               exit_use=exit_use, hotspots=hotspots)
    return out


def build_maps(counts: dict, steps, episodes, bad: int) -> dict:
    """``SpatialMaps.maps()`` from host arrays, no device: ``counts`` the five [n_rows, GX, GY]
    int64 arrays (``arrive``, ``stall``, ``evac``, ``died``, ``robot``), ``steps`` / ``episodes``
    [n_rows].

    Returns ``bad`` and one entry per row under its index plus ``"sum"`` (the rows added up, exact).
    An entry holds the five arrays [GX, GY]; ``occupancy`` = arrive + stall (live persons per cell
    after a step); ``steps`` (env-steps folded) and ``episodes`` (finished ones among them);
    ``density`` = occupancy / steps (NaN without a step); ``stall_ratio`` = stall / occupancy, NaN
    where occupancy is 0; ``exit_use`` = [(x, y, count, share)] over the cells with evac > 0,
    largest count first and ties by cell index (x * GY + y); ``hotspots`` = [(x, y, stall)] of the
    10 cells with the largest stall > 0, ties by cell index."""
    tabs = {k: np.asarray(counts[k], np.int64) for k in MAP_FIELDS}
    steps, episodes = np.asarray(steps, np.int64).reshape(-1), np.asarray(episodes, np.int64).reshape(-1)
    out = {r: _row_maps({k: v[r] for k, v in tabs.items()}, steps[r], episodes[r]) for r in range(len(steps))}
    out["sum"] = _row_maps({k: v.sum(axis=0) for k, v in tabs.items()}, steps.sum(), episodes.sum())
    out["bad"] = int(bad)
    return out


def plan(GX: int, GY: int, P: int, n_rows: int = 1) -> dict:
    """``evx_spatial_plan``: the route (``"LDS"`` / ``"BANDS"``) and launch shape an update of this
    grid takes, as the launcher decides it. No launch, no device."""
    pl = evx_spatial_launch()
    check(lib().evx_spatial_plan(int(GX), int(GY), int(P), int(n_rows), C.byref(pl)), "spatial_plan")
    out = {name: int(getattr(pl, name)) for name, _ in evx_spatial_launch._fields_}
    out["route"] = {v: k for k, v in SPATIAL.items()}[pl.route]
    return out


class SpatialMaps:
    """Spatial maps of E envs of ``layout`` (a DeviceLayout, a LayoutSet, or a ``Grid``: anything
    with GX, GY, P, R).

    layout_idx / n_layouts / cap are EpisodeStats's: one row of maps per layout, and with cap > 0
    only the first ``cap`` episodes of every env are counted.

    Public tensors: ``prev`` [E, P] (each env's ``pk`` as of the previous state), ``n_total`` [E],
    ``arrive``, ``stall``, ``evac``, ``died``, ``robot`` [n_layouts, GX, GY], ``steps``
    [n_layouts], ``bad`` [1]."""

    def __init__(self, E: int, device, layout, layout_idx: Optional[torch.Tensor] = None, n_layouts: int = 1,
                 cap: int = 0):
        E, n_layouts, cap = int(E), int(n_layouts), int(cap)
        GX, GY, P, R = (int(getattr(layout, k)) for k in ("GX", "GY", "P", "R"))
        if E < 1 or not 1 <= P <= MAX_P or R < 0:
            raise ValueError(f"SpatialMaps: E must be >= 1, P 1..{MAX_P} and R >= 0, not {E}, {P}, {R}")
        if not (1 <= GX <= SPATIAL_MAX_GRID and 1 <= GY <= SPATIAL_MAX_GRID):
            raise ValueError(f"SpatialMaps: GX and GY must be 1..{SPATIAL_MAX_GRID}, not {GX}, {GY}")
        if cap < 0:
            raise ValueError("SpatialMaps: cap must be >= 0")
        device = check_rows("SpatialMaps", E, n_layouts, layout_idx, device, where="the maps are")
        self.E, self.P, self.R, self.GX, self.GY, self.n_layouts, self.cap = E, P, R, GX, GY, n_layouts, cap
        self.layout_idx = layout_idx
        i64 = dict(dtype=torch.int64, device=device)
        self.prev = torch.zeros(E, P, dtype=torch.int32, device=device)
        self.n_total = torch.zeros(E, **i64)
        for name in MAP_FIELDS:
            setattr(self, name, torch.zeros(n_layouts, GX, GY, **i64))
        self.steps = torch.zeros(n_layouts, **i64)
        self.bad = torch.zeros(1, **i64)
        self.device = self.prev.device  # with its index
        self.c = evx_spatial(E=E, P=P, R=R, GX=GX, GY=GY, n_rows=n_layouts)
        for name in ("prev", "n_total", *MAP_FIELDS, "steps", "bad"):
            setattr(self.c, name, _ptr(getattr(self, name)))
        check(lib().evx_spatial_init(C.byref(self.c), _stream()), "spatial_init")

    def _state(self, env_or_tensors):
        if isinstance(env_or_tensors, (tuple, list)):
            pk, robots = env_or_tensors
        else:
            pk, robots = env_or_tensors.pk, env_or_tensors.robots
        need("pk", pk, self.E * self.P, torch.int32, self.device)
        if self.R:
            need("robots", robots, self.E * self.R, torch.int32, self.device)
        else:
            robots = None
        return pk, robots

    def sync(self, env, mask: Optional[torch.Tensor] = None):
        """``prev`` takes ``pk`` for the envs with mask != 0 (None: every env): call it after the
        first reset and after every masked reset. ``env`` is a VecEnv, pk itself (int32 [E, P]) or a
        pair that starts with it. One launch on the current stream."""
        pk = env if isinstance(env, torch.Tensor) else env[0] if isinstance(env, (tuple, list)) else env.pk
        need("pk", pk, self.E * self.P, torch.int32, self.device)
        if mask is not None:
            need("mask", mask, self.E, torch.uint8, self.device)
        check(lib().evx_spatial_sync(C.byref(self.c), pk.data_ptr(), _ptr(mask), _stream()), "spatial_sync")

    def update(self, env, done: torch.Tensor):
        """Count one step of every env: ``env`` is a VecEnv (its ``pk`` and ``robots``) or a pair
        (pk int32 [E, P], robots int32 [E, R] or None with R = 0) as the step left them and before
        any reset; ``done`` the step's output. One launch on the current stream, two on the banded
        route (``plan()``)."""
        pk, robots = self._state(env)
        need("done", done, self.E, torch.uint8, self.device)
        check(lib().evx_spatial_update(C.byref(self.c), pk.data_ptr(), _ptr(robots), done.data_ptr(),
                                       _ptr(self.layout_idx), self.cap, _stream()), "spatial_update")

    def plan(self) -> dict:
        """The route and launch shape ``update`` takes (``evx_spatial_plan``)."""
        return plan(self.GX, self.GY, self.P, self.n_layouts)

    def episodes(self) -> np.ndarray:
        """Finished episodes counted per row [n_layouts]: every env's ``n_total``, at most ``cap``."""
        n = self.n_total.cpu().numpy()
        n = np.minimum(n, self.cap) if self.cap > 0 else n
        rows = np.zeros(self.E, np.int64) if self.layout_idx is None else \
            np.clip(self.layout_idx.cpu().numpy().astype(np.int64), 0, self.n_layouts - 1)
        return np.bincount(rows, weights=n, minlength=self.n_layouts).astype(np.int64)

    def maps(self) -> dict:
        """Copy the counts to the host (this waits for the current stream) and return
        ``build_maps`` of them: plain numpy."""
        counts = {k: getattr(self, k).cpu().numpy() for k in MAP_FIELDS}
        return build_maps(counts, self.steps.cpu().numpy(), self.episodes(), int(self.bad.item()))


__all__ = ["Grid", "SpatialMaps", "build_maps", "plan", "evx_spatial", "MAP_FIELDS"]
