"""Population-based training on a PopulationTrainer: the exploit / explore scheduler.

At intervals the worst members of a population take the weights and the hyperparameters of the
best ones and perturb the hyperparameters (Jaderberg et al. 2017, "Population Based Training of
Neural Networks"). ``PBTScheduler`` is the host side of that: it keeps its own window of the
members' episode counts and sums (``observe``), ranks the members (``plan``) and hands the result
to the trainer (``apply``: ``set_hparams`` per receiver, then one ``copy_members`` launch). Nothing
here touches a device before ``apply``, and nothing waits for one: the only host sync of a round is
the ``episode_summary()`` the caller made anyway for its log line.

A plan is a pure function of (seed, round, the window, the hyperparameters): receiver k draws from
``numpy.random.default_rng([seed, round, k])``, its donor first, then one draw per name of the
space in sorted order.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence, Union

import numpy as np

from ._lib import NSTEP_MAX
from .population import _HP, _OPT, MAX_MEMBERS, per_member

NAMES = _HP + _OPT  # what set_hparams takes
INT_NAMES = ("n_step", "target_every")
WINDOW_KEYS = ("episodes", "return_sum", "evacuated", "dead")
FITNESS = ("return_mean", "evac_rate", "neg_death_rate")


def _number(what: str, x) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
        raise ValueError(f"{what} must be a finite number, not {x!r}")
    return float(x)


def check_space(space) -> dict:
    """The search space as the scheduler keeps it: name -> ("perturb", factors, lo, hi) or
    ("resample", values), tuples throughout. ValueError naming the entry for an unknown name, a
    malformed spec, ``loss`` with "perturb", a factor that is not a finite number > 0, lo > hi, a
    bound or a resample value that set_hparams would refuse."""
    if not isinstance(space, dict):
        raise ValueError(f"space must be a dict from a hyperparameter name to a spec, not {space!r}")
    out = {}
    for name, spec in space.items():
        if name not in NAMES:
            raise ValueError(f"space: unknown hyperparameter {name!r} (one of {', '.join(NAMES)})")
        if not isinstance(spec, (list, tuple)) or not spec or spec[0] not in ("perturb", "resample"):
            raise ValueError(f"space[{name!r}] must be ('perturb', factors, lo, hi) or ('resample', values), "
                             f"not {spec!r}")
        if spec[0] == "resample":
            if len(spec) != 2 or not isinstance(spec[1], (list, tuple)) or not spec[1]:
                raise ValueError(f"space[{name!r}]: ('resample', values) needs a non-empty sequence of values, "
                                 f"not {spec!r}")
            out[name] = ("resample", tuple(per_member(name, v, 1)[0] for v in spec[1]))
            continue
        if name == "loss":
            raise ValueError("space['loss']: a loss is a name, not a number: ('resample', values) only")
        if len(spec) != 4 or not isinstance(spec[1], (list, tuple)) or not spec[1]:
            raise ValueError(f"space[{name!r}]: ('perturb', factors, lo, hi) needs a non-empty sequence of factors "
                             f"and two bounds, not {spec!r}")
        factors = tuple(_number(f"space[{name!r}]: a factor", f) for f in spec[1])
        if min(factors) <= 0:
            raise ValueError(f"space[{name!r}]: a factor must be > 0, not {min(factors)!r}")
        lo, hi = _number(f"space[{name!r}]: lo", spec[2]), _number(f"space[{name!r}]: hi", spec[3])
        if lo > hi:
            raise ValueError(f"space[{name!r}]: lo = {lo!r} is above hi = {hi!r}")
        if name not in INT_NAMES:  # (an integer name is rounded into its own range afterwards)
            per_member(name, lo, 1)
            per_member(name, hi, 1)
        out[name] = ("perturb", factors, lo, hi)
    return out


class PBTScheduler:
    def __init__(self, members: int, space: dict, frac: float = 0.25, min_episodes: int = 1,
                 fitness: Union[str, Callable[[dict], float]] = "return_mean", seed: int = 0,
                 people: Optional[int] = None):
        """members = K of the trainer. space: check_space's dict. frac: the share of the population
        replaced per round, in [0, 1]. min_episodes >= 1: a member with fewer finished episodes in the
        window takes no part in a round. fitness, higher is better: "return_mean" (return_sum /
        episodes), "evac_rate" and "neg_death_rate" (evacuated, -dead per episode and person; people
        None: per episode, the same ranking since the members share one layout), or a callable from a
        member's window dict (episodes, return_sum, evacuated, dead) to a float. seed >= 0 keys the
        draws."""
        if isinstance(members, bool) or not isinstance(members, int) or not 1 <= members <= MAX_MEMBERS:
            raise ValueError(f"members must be an integer in 1..{MAX_MEMBERS}, not {members!r}")
        self.frac = _number("frac", frac)
        if not 0 <= self.frac <= 1:
            raise ValueError(f"frac must lie in [0, 1], not {frac!r}")
        if isinstance(min_episodes, bool) or not isinstance(min_episodes, int) or min_episodes < 1:
            raise ValueError(f"min_episodes must be an integer >= 1, not {min_episodes!r}")
        if not callable(fitness) and fitness not in FITNESS:
            raise ValueError(f"fitness must be one of {', '.join(FITNESS)} or a callable, not {fitness!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or seed < 0:
            raise ValueError(f"seed must be an integer >= 0, not {seed!r}")
        if people is not None and (isinstance(people, bool) or not isinstance(people, int) or people < 1):
            raise ValueError(f"people must be an integer >= 1, not {people!r}")
        self.K, self.space, self.min_episodes, self.fitness = members, check_space(space), min_episodes, fitness
        self.seed, self.people, self.round = seed, people, 0
        self.clear()

    # ---------------------------------------------------------------- window
    def clear(self):
        self.window = [dict(episodes=0, return_sum=0.0, evacuated=0, dead=0) for _ in range(self.K)]

    def observe(self, summary: dict):
        """Add an episode_summary() dict (its per_member rows) to the window. The scheduler never asks
        the trainer for a summary itself: the caller's log window stays the caller's."""
        rows = summary.get("per_member") if isinstance(summary, dict) else None
        if rows is None or len(rows) != self.K:
            raise ValueError(f"observe: an episode_summary() dict with per_member of {self.K} members is needed")
        for w, row in zip(self.window, rows):
            for key in WINDOW_KEYS:
                w[key] += row[key]

    def member_fitness(self, k: int) -> Optional[float]:
        """Member k's fitness over the window; None if it is not eligible (fewer than min_episodes
        episodes, or a fitness that is not finite)."""
        w = self.window[k]
        n = w["episodes"]
        if n < self.min_episodes:
            return None
        per = n * (self.people or 1)
        if callable(self.fitness):
            f = self.fitness(dict(w))
        elif self.fitness == "return_mean":
            f = w["return_sum"] / n
        elif self.fitness == "evac_rate":
            f = w["evacuated"] / per
        else:
            f = -w["dead"] / per
        try:
            f = float(f)
        except (TypeError, ValueError):
            return None
        return f if math.isfinite(f) else None

    # ------------------------------------------------------------------ plan
    def _explore(self, name, base, rng, n_step_max):
        spec = self.space[name]
        if spec[0] == "resample":
            return spec[1][int(rng.integers(len(spec[1])))]
        _, factors, lo, hi = spec
        v = min(max(float(base) * factors[int(rng.integers(len(factors)))], lo), hi)
        if name not in INT_NAMES:
            return v
        v = max(1, int(math.floor(v + 0.5)))
        return min(v, n_step_max) if name == "n_step" else v

    def plan(self, hparams, n_step_max: Optional[int] = None) -> List[dict]:
        """One round's decisions from the window, then the window is cleared and ``round`` advances
        (also when nothing is replaced). hparams: the current values of every name of the space, K
        per name -- a PopulationTrainer, or a dict of lists. n_step_max: the deepest chain the
        trainer's ring holds (round_ passes it); n_step is capped by it and by NSTEP_MAX.

        The eligible members are ranked by (fitness descending, index ascending); q = min(floor(frac
        K), eligible // 2); the last q are receivers, the first q donors, so no member is both.
        Receiver k draws its donor, inherits the donor's value of every name of the space and explores
        it. Each decision: dst, src, fitness_dst, fitness_src, and old / new, the receiver's values per
        name before and after."""
        cap = NSTEP_MAX if n_step_max is None else max(1, min(NSTEP_MAX, int(n_step_max)))
        get = (lambda name: hparams[name]) if isinstance(hparams, dict) else (lambda name: getattr(hparams, name))
        cur = {name: list(get(name)) for name in self.space}
        for name, vals in cur.items():
            if len(vals) != self.K:
                raise ValueError(f"plan: {name} holds {len(vals)} values for {self.K} members")
        fit = [self.member_fitness(k) for k in range(self.K)]
        ranking = sorted((k for k in range(self.K) if fit[k] is not None), key=lambda k: (-fit[k], k))
        q = min(int(math.floor(self.frac * self.K)), len(ranking) // 2)
        donors, receivers = ranking[:q], ranking[len(ranking) - q:] if q else []
        decisions = []
        for k in receivers:
            rng = np.random.default_rng([self.seed, self.round, k])
            src = donors[int(rng.integers(q))]
            new = {name: self._explore(name, cur[name][src], rng, cap) for name in sorted(self.space)}
            decisions.append(dict(dst=k, src=src, fitness_dst=fit[k], fitness_src=fit[src],
                                  old={name: cur[name][k] for name in sorted(self.space)}, new=new))
        self.clear()
        self.round += 1
        return decisions

    def src_map(self, decisions: Sequence[dict]) -> List[int]:
        """The decisions as copy_members' map: src_map[dst] = src, every other member itself."""
        m = list(range(self.K))
        for d in decisions:
            m[d["dst"]] = d["src"]
        return m

    # ----------------------------------------------------------------- apply
    def apply(self, trainer, decisions: Sequence[dict]):
        """Hand a plan to the trainer: set_hparams for each receiver, then one copy_members launch
        on the current stream. No host sync; an empty plan does nothing."""
        if trainer.K != self.K:
            raise ValueError(f"apply: the trainer has {trainer.K} members, the scheduler {self.K}")
        if not decisions:
            return
        for d in decisions:
            trainer.set_hparams(d["dst"], **d["new"])
        trainer.copy_members(self.src_map(decisions))

    def round_(self, trainer) -> List[dict]:
        """plan + apply on a PopulationTrainer; returns the decisions."""
        decisions = self.plan(trainer, n_step_max=trainer.replay.capacity // trainer.N)
        self.apply(trainer, decisions)
        return decisions


def parse_space(text: str) -> dict:
    """A search space from the runner's flag: entries joined by ';', each name:perturb:factors:lo:hi
    or name:resample:values, lists joined by ',' -- lr:perturb:0.8,1.25:1e-6:1e-2;n_step:resample:1,3,5.
    Values of n_step and target_every are read as integers, loss as names, the others as floats."""
    space = {}
    for entry in (e.strip() for e in str(text).split(";")):
        if not entry:
            continue
        parts = [p.strip() for p in entry.split(":")]
        name = parts[0]
        if name in space:
            raise ValueError(f"--pbt-space: {name!r} is given twice")
        try:
            if len(parts) == 5 and parts[1] == "perturb":
                space[name] = ("perturb", [float(x) for x in parts[2].split(",")], float(parts[3]), float(parts[4]))
            elif len(parts) == 3 and parts[1] == "resample":
                conv = str if name == "loss" else int if name in INT_NAMES else float
                space[name] = ("resample", [conv(x.strip()) for x in parts[2].split(",")])
            else:
                raise ValueError
        except ValueError:
            raise ValueError(f"--pbt-space: cannot read {entry!r} (name:perturb:factors:lo:hi or "
                             f"name:resample:values)") from None
    return check_space(space)


__all__ = ["PBTScheduler", "check_space", "parse_space", "FITNESS"]
