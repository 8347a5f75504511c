"""Evaluate a policy over many envs on the device.

The reference's runners/evaluate_strategies.py:47-77 steps one env from Python per
strategy and averages the episodes' rewards and rates on the host. ``evaluate`` runs E
envs with auto-reset and an ``EpisodeStats(cap=episodes_per_env)``, so exactly the first
``episodes_per_env`` episodes of every env are counted (short episodes are not
over-represented), and looks at the device only every ``check_every`` steps.

``metrics=True`` adds the reference's per-episode health metrics
(EvacuationEnv.get_performance_metrics, envs/evacuation_env.py:290-309) through
``evacx.health.HealthStats``; ``timeline=True`` adds the per-step evacuation curves and tracked
persons of the reference's recorded evaluation episode (``evacx.timeline.Timeline``);
``maps=True`` adds where it happened -- occupancy, stalls, exit use, deaths and robot positions per
grid cell (``evacx.spatial.SpatialMaps``); ``policy="greedy"`` also takes one network per robot (a
GroupedLearner, a GroupedQMix, or a sequence of Learners).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from .env import OBS_WORDS, VecEnv, _stream, n_layout_rows
from .episodes import EpisodeStats

N_ACTIONS = 5
EPISODE_MAX_STEPS = 1200  # max_simulation_time / time_per_step (envs/evacuation_env.py:26-28)
TIME_PER_STEP = 0.5       # envs/evacuation_env.py:27


def _check_policy(policy, learner):
    if isinstance(policy, bool) or not isinstance(policy, (str, int)):
        raise ValueError(f"policy must be 'greedy', 'random' or an action index, not {policy!r}")
    if isinstance(policy, str):
        if policy not in ("greedy", "random"):
            raise ValueError(f"policy must be 'greedy', 'random' or an action index, not {policy!r}")
        if policy == "greedy" and learner is None:
            raise ValueError("policy 'greedy' needs a learner (evacx.qnet.Learner)")
    elif not 0 <= policy < N_ACTIONS:
        raise ValueError(f"a constant policy must be an action 0..{N_ACTIONS - 1}, not {policy}")


def _check_table(fast, layout):
    if fast is not None and getattr(fast, "_static", None) is not None and fast._static[0] is not layout.c:
        raise ValueError("evaluate: the learner's act table was attached for another layout")


def _same_device(a, b) -> bool:
    a, b = torch.device(a), torch.device(b)
    return a.type == b.type and (a.index or 0) == (b.index or 0)


def _multi_agent(learner, layout, E: int):
    """("grouped", GroupedLearner) / ("each", [Learner] * R) for a per-robot ``learner``, None for a
    single shared one; refuses a wrong count, an odd E or another device (ValueError)."""
    from .qgroup import GroupedLearner, GroupedQMix
    if isinstance(learner, GroupedQMix):
        learner = learner.A  # the mixer plays no part in acting
    if isinstance(learner, GroupedLearner):
        kind, nets, devs = "grouped", learner.G, [learner.device]
    elif isinstance(learner, (list, tuple)):
        kind, nets, devs = "each", len(learner), [lr.device for lr in learner]
        learner = list(learner)
    else:
        return None
    if nets != layout.R:
        raise ValueError(f"learner: {nets} networks for a layout of {layout.R} robots (one per robot is needed)")
    if E % 2:
        raise ValueError(f"E: the per-robot acts take an even number of envs (dropout row pairs), not {E}")
    for d in devs:
        if not _same_device(d, layout.device):
            raise ValueError(f"learner: a network on {d}, the layout is on {layout.device}")
    return kind, learner


class _EachRobot:
    """One Learner per robot: robot r's observation rows (env * R + r) are gathered
    (evx_gather_obs), run through learner r in eval mode and the actions scattered back."""

    def __init__(self, learners, layout, E: int):
        self.learners, self.lay, self.E, self.R = learners, layout, E, layout.R
        for lr in learners:
            _check_table(getattr(lr, "fast", None), layout)
        dev = layout.device
        self.idx = [(torch.arange(E, dtype=torch.int64, device=dev) * self.R + r).contiguous() for r in range(self.R)]
        self.obs = torch.zeros(E * OBS_WORDS, dtype=torch.int32, device=dev)
        self.act_r = torch.zeros(E, dtype=torch.int32, device=dev)

    def __call__(self, env, actions, seed: int, offset: int):
        E, lay = self.E, self.lay
        for r, lr in enumerate(self.learners):
            _lib.check(_lib.lib().evx_gather_obs(env.obs.data_ptr(), self.idx[r].data_ptr(), E, self.obs.data_ptr(),
                                                 _stream()), "gather_obs")
            fast = getattr(lr, "fast", None)
            if fast is not None:
                fast.act(lay.c, self.obs, E, drop=None, actions=self.act_r, epsilon=0.0, act_seed=seed,
                         act_offset=offset + r * E)
            else:
                x = torch.empty((E, 11, 11, 6), dtype=torch.float32, device=lay.device)
                _lib.check(_lib.lib().evx_obs_expand_f32(C.byref(lay.c), self.obs.data_ptr(), E, x.data_ptr(),
                                                         _stream()), "evx_obs_expand")
                Q = lr.q_values(x, train=False, tag="eval")
                _lib.check(_lib.lib().evx_act(Q.data_ptr(), E, lr.actions, 0.0, seed, offset + r * E,
                                              self.act_r.data_ptr(), _stream()), "act")
            actions.view(E, self.R)[:, r].copy_(self.act_r)


def evaluate(layout, E: int, episodes_per_env: int, policy, learner=None, seed_base: int = 1234, seed: int = 0,
             check_every: int = 16, max_steps: Optional[int] = None, layout_of: Optional[Sequence[int]] = None,
             metrics: bool = False, timeline: bool = False, track=None, maps: bool = False) -> dict:
    """Run E envs of ``layout`` (a DeviceLayout, or a LayoutSet with ``layout_of``) under
    ``policy`` until every env has finished ``episodes_per_env`` episodes, and return the
    EpisodeStats summary over exactly E * episodes_per_env episodes, with ``per_env`` = the
    per-env tensors (window sums, ``n_total``, and the episode table ``tab_ret`` / ``tab_len``
    / ``tab_evac`` / ``tab_dead`` [E, episodes_per_env] in episode order) and ``steps``.

    policy: ``"greedy"`` -- argmax of ``learner``'s online net in eval mode (dropout p = 0,
    epsilon 0), through the fused act kernel where the learner has it, else q_values + evx_act;
    ``"random"`` -- evx_act with epsilon 1: uniform actions from its counter RNG (key ``seed``,
    counter step * E * R + robot row); an int a -- every robot takes action a every step.
    For ``"greedy"``, ``learner`` is an evacx.qnet.Learner shared by every robot, or one network
    per robot: a GroupedLearner or a GroupedQMix (its agents) of ``layout.R`` nets -- robot r of
    every env through net r, one evx_qmlp_act_g launch per step -- or a sequence of ``layout.R``
    Learners of either kind (robot r's rows gathered, run through learner r, scattered back).
    The per-robot forms need an even E.
    Env seeds are seed_base + env, as in VecTrainer. The number of unfinished envs is read
    every ``check_every`` steps (the only host sync); more than ``max_steps`` steps (default
    episodes_per_env * 1200, the env's own step limit) raise RuntimeError.

    metrics=True: the envs step with resets apart (``auto_reset=False``, then
    ``env.reset(mask=env.done)`` with the device mask; the same trajectory), and between the two a
    ``HealthStats`` takes every finished episode's terminal health. The result gains
    ``avg_health`` (mean over the episodes with somebody alive; None without one),
    ``min_health`` (the smallest), ``min_health_mean``, ``alive_mean``, ``health_episodes``,
    ``total_time_mean`` (= ``length_mean`` * 0.5, the env's time_per_step), and ``per_env`` the
    table ``tab_avg_health`` / ``tab_min_health`` / ``tab_alive``. No host sync is added.

    timeline=True: the same reset-apart path, with an ``evacx.timeline.Timeline`` (T = 1200, the
    env's step limit; cap = episodes_per_env) counting every step between the step and the reset,
    after the health update where both are asked for. The result gains ``curves``
    (``Timeline.curves()``: per-step evacuated / dead / remaining / avg_health curves, the
    evacuation-time and death-time distributions, per layout and summed). ``track`` = a person
    count n (the first n persons of env 0) or (env_ids, person_ids) also keeps those persons'
    positions and health over their env's first episode (``curves["tracked"]``); it needs
    ``timeline=True`` (ValueError). No host sync is added.

    maps=True: the same reset-apart path, with an ``evacx.spatial.SpatialMaps`` (cap =
    episodes_per_env) that is synced after the first reset, counts every step between the step and
    the reset, after the health and timeline updates, and is synced again for the envs the masked
    reset restarted. The result gains ``maps`` (``SpatialMaps.maps()``: per layout and summed, the
    arrive / stall / evac / died / robot counts per grid cell, occupancy, density, the stall ratio,
    the exits' shares and the stall hotspots). No host sync is added; with maps=False nothing is
    allocated or launched."""
    _check_policy(policy, learner)
    if track is not None and not timeline:
        raise ValueError("evaluate: track needs timeline=True")
    E, K, check_every = int(E), int(episodes_per_env), int(check_every)
    if E < 1 or K < 1 or check_every < 1:
        raise ValueError("evaluate: E, episodes_per_env and check_every must be >= 1")
    max_steps = K * EPISODE_MAX_STEPS if max_steps is None else int(max_steps)
    multi = _multi_agent(learner, layout, E) if policy == "greedy" else None
    fast = getattr(learner, "fast", None) if policy == "greedy" and multi is None else None
    _check_table(fast, layout)

    env = VecEnv(layout, E, layout_of=layout_of)
    env.seed([seed_base + i for i in range(E)])
    env.reset()
    n_layouts = n_layout_rows(layout)
    stats = EpisodeStats(E, layout.device, layout.P, layout_idx=env.layout_idx, n_layouts=n_layouts, cap=K, record=K)
    health = None
    if metrics:
        from .health import HealthStats
        health = HealthStats(E, layout.device, layout.P, layout_idx=env.layout_idx, n_layouts=n_layouts, cap=K,
                             record=K)
    tline = None
    if timeline:
        from .timeline import Timeline
        tline = Timeline(E, layout.device, layout.P, T=EPISODE_MAX_STEPS, layout_idx=env.layout_idx,
                         n_layouts=n_layouts, cap=K, track=track)
        tline.trace0(env)
    smaps = None
    if maps:
        from .spatial import SpatialMaps
        smaps = SpatialMaps(E, layout.device, layout, layout_idx=env.layout_idx, n_layouts=n_layouts, cap=K)
        smaps.sync(env)
    n = E * layout.R
    actions = torch.full((n,), policy if isinstance(policy, int) else 0, dtype=torch.int32, device=layout.device)
    q0 = torch.zeros(n, N_ACTIONS, dtype=torch.float32, device=layout.device) if policy == "random" else None
    each = _EachRobot(multi[1], layout, E) if multi is not None and multi[0] == "each" else None
    steps, out = 0, None
    while out is None:
        if steps >= max_steps:
            raise RuntimeError(f"evaluate: {stats.summary(clear=False)['remaining']} envs have not finished "
                               f"{K} episodes after {steps} steps")
        if policy == "random":
            _lib.check(_lib.lib().evx_act(q0.data_ptr(), n, N_ACTIONS, 1.0, seed, steps * n, actions.data_ptr(),
                                          _stream()), "act")
        elif each is not None:
            each(env, actions, seed, steps * n)
        elif multi is not None:
            multi[1].act(layout.c, env.obs, E, actions=actions, epsilon=0.0, act_seed=seed, act_offset=steps * n,
                         drop_p=0.0, drop_stream=0)
        elif fast is not None:
            fast.act(layout.c, env.obs, n, drop=None, actions=actions, epsilon=0.0, act_seed=seed, act_offset=steps * n)
        elif policy == "greedy":
            x = env.expand_obs(torch.float32)
            Q = learner.q_values(x.view(n, 11, 11, 6), train=False, tag="eval")
            _lib.check(_lib.lib().evx_act(Q.data_ptr(), n, learner.actions, 0.0, seed, steps * n, actions.data_ptr(),
                                          _stream()), "act")
        if health is None and tline is None and smaps is None:
            env.step(actions, auto_reset=True)
            stats.update(env.reward, env.done, env.counts)
        else:  # the state the step left is read between the step and the reset
            env.step(actions, auto_reset=False)
            if health is not None:
                health.update(env, env.done)
            if tline is not None:
                tline.update(env, env.done, env.counts)
            if smaps is not None:
                smaps.update(env, env.done)
            stats.update(env.reward, env.done, env.counts)
            env.reset(mask=env.done)
            if smaps is not None:
                smaps.sync(env, mask=env.done)
        steps += 1
        if steps % check_every == 0 or steps >= max_steps:
            s = stats.summary(clear=False)
            if s["remaining"] == 0:
                out = s
    env.check_err()
    out["steps"] = steps
    out["per_env"] = {k: getattr(stats, k) for k in ("n_total", "w_n", "w_len", "w_evac", "w_dead", "w_ret", "w_ret2",
                                                     "w_min", "w_max", "tab_ret", "tab_len", "tab_evac", "tab_dead")}
    if health is not None:
        h = health.summary(clear=False)
        for k in ("avg_health", "min_health", "min_health_mean", "alive_mean", "health_episodes"):
            out[k] = h[k]
        out["total_time_mean"] = None if out["length_mean"] is None else out["length_mean"] * TIME_PER_STEP
        for k, hl in zip(out["per_layout"], h["per_layout"]):
            for name in ("avg_health", "min_health", "min_health_mean", "alive_mean", "health_episodes"):
                k[name] = hl[name]
        out["per_env"].update(tab_avg_health=health.tab_avg, tab_min_health=health.tab_min,
                              tab_alive=health.tab_alive)
    if tline is not None:
        out["curves"] = tline.curves()
    if smaps is not None:
        out["maps"] = smaps.maps()
    return out


__all__ = ["evaluate"]
