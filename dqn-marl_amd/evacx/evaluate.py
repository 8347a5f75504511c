"""Evaluate a policy over many envs on the device.

The reference's runners/evaluate_strategies.py:47-77 steps one env from Python per
strategy and averages the episodes' rewards and rates on the host. ``evaluate`` runs E
envs with auto-reset and an ``EpisodeStats(cap=episodes_per_env)``, so exactly the first
``episodes_per_env`` episodes of every env are counted (short episodes are not
over-represented), and looks at the device only every ``check_every`` steps.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .env import VecEnv, _stream
from .episodes import EpisodeStats

N_ACTIONS = 5
EPISODE_MAX_STEPS = 1200  # max_simulation_time / time_per_step (envs/evacuation_env.py:26-28)


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


def evaluate(layout, E: int, episodes_per_env: int, policy, learner=None, seed_base: int = 1234, seed: int = 0,
             check_every: int = 16, max_steps: Optional[int] = None, layout_of: Optional[Sequence[int]] = None) -> dict:
    """Run E envs of ``layout`` (a DeviceLayout, or a LayoutSet with ``layout_of``) under
    ``policy`` until every env has finished ``episodes_per_env`` episodes, and return the
    EpisodeStats summary over exactly E * episodes_per_env episodes, with ``per_env`` = the
    per-env tensors (window sums, ``n_total``, and the episode table ``tab_ret`` / ``tab_len``
    / ``tab_evac`` / ``tab_dead`` [E, episodes_per_env] in episode order) and ``steps``.

    policy: ``"greedy"`` -- argmax of ``learner``'s online net in eval mode (dropout p = 0,
    epsilon 0), through the fused act kernel where the learner has it, else q_values + evx_act;
    ``"random"`` -- evx_act with epsilon 1: uniform actions from its counter RNG (key ``seed``,
    counter step * E * R + robot row); an int a -- every robot takes action a every step.
    Env seeds are seed_base + env, as in VecTrainer. The number of unfinished envs is read
    every ``check_every`` steps (the only host sync); more than ``max_steps`` steps (default
    episodes_per_env * 1200, the env's own step limit) raise RuntimeError."""
    _check_policy(policy, learner)
    E, K, check_every = int(E), int(episodes_per_env), int(check_every)
    if E < 1 or K < 1 or check_every < 1:
        raise ValueError("evaluate: E, episodes_per_env and check_every must be >= 1")
    max_steps = K * EPISODE_MAX_STEPS if max_steps is None else int(max_steps)
    fast = getattr(learner, "fast", None) if policy == "greedy" else None
    if fast is not None and getattr(fast, "_static", None) is not None and fast._static[0] is not layout.c:
        raise ValueError("evaluate: the learner's act table was attached for another layout")
    from .qnet import qcheck, qlib

    env = VecEnv(layout, E, layout_of=layout_of)
    env.seed([seed_base + i for i in range(E)])
    env.reset()
    stats = EpisodeStats(E, layout.device, layout.P, layout_idx=env.layout_idx,
                         n_layouts=len(layout.layouts) if hasattr(layout, "layouts") else 1, cap=K, record=K)
    n = E * layout.R
    actions = torch.full((n,), policy if isinstance(policy, int) else 0, dtype=torch.int32, device=layout.device)
    q0 = torch.zeros(n, N_ACTIONS, dtype=torch.float32, device=layout.device) if policy == "random" else None
    steps, out = 0, None
    while out is None:
        if steps >= max_steps:
            raise RuntimeError(f"evaluate: {stats.summary(clear=False)['remaining']} envs have not finished "
                               f"{K} episodes after {steps} steps")
        if policy == "random":
            qcheck(qlib().evx_act(q0.data_ptr(), n, N_ACTIONS, 1.0, seed, steps * n, actions.data_ptr(), _stream()),
                   "act")
        elif fast is not None:
            fast.act(layout.c, env.obs, n, drop=None, actions=actions, epsilon=0.0, act_seed=seed, act_offset=steps * n)
        elif policy == "greedy":
            x = env.expand_obs(torch.float32)
            Q = learner.q_values(x.view(n, 11, 11, 6), train=False, tag="eval")
            qcheck(qlib().evx_act(Q.data_ptr(), n, learner.actions, 0.0, seed, steps * n, actions.data_ptr(),
                                  _stream()), "act")
        env.step(actions, auto_reset=True)
        stats.update(env.reward, env.done, env.counts)
        steps += 1
        if steps % check_every == 0 or steps >= max_steps:
            s = stats.summary(clear=False)
            if s["remaining"] == 0:
                out = s
    env.check_err()
    out["steps"] = steps
    out["per_env"] = {k: getattr(stats, k) for k in ("n_total", "w_n", "w_len", "w_evac", "w_dead", "w_ret", "w_ret2",
                                                     "w_min", "w_max", "tab_ret", "tab_len", "tab_evac", "tab_dead")}
    return out


__all__ = ["evaluate"]
