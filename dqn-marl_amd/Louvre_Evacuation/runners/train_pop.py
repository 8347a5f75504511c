"""Population training: K independent DQN learners (seeds, learning rates, discounts, exploration
schedules) in one process, every step in grouped launches (evacx.population.PopulationTrainer).

What the reference's runners/overnight_experiments.py does one run after another: the same
training over several seeds and hyperparameters, ranked by death rate, then evacuation rate.
Reads the env and agent sections of ``configs/dqn.yaml`` as train_vec does; ``--lr``, ``--gamma``,
``--epsilon-decay``, ``--target-every`` and ``--seeds`` take one value for every member or K
comma-separated values (default: the config's agent keys; seeds: ``--seed`` + k). ``--envs`` is the
total over members (a multiple of K). ``--loss``, ``--huber-delta``, ``--target-tau`` and ``--n-step``
are comma lists in the same way (defaults: the optional ``agent:`` keys train_vec reads);
``--double-q`` holds for every member. The ring is sized for the deepest member's n_step pushes. Every ``--log-every`` steps one ``episode_summary()``:

  member<k>/training_log.csv   train_vec's columns, member k's envs
  population_summary.csv       per log line the mean, std, min and max over members of return,
                               evacuation rate and death rate, and the best member's index
  member<k>/dqn_model.pth      the reference's checkpoint dict (loads with evaluate_vec --dqn)
  best_member.json             the best member of the last window: lowest death rate, then highest
                               evacuation rate (overnight_experiments.py's ordering), with its values

``--eval-episodes N`` ends with a greedy evaluation (evacx.evaluate) of every member.

``--pbt-every N`` (a multiple of ``--log-every``; 0, the default: off, the run above exactly) turns
the grid into population-based training (evacx.pbt.PBTScheduler): every log line's summary goes to
the scheduler, and right after the log line of every N-th step the worst ``--pbt-frac`` of the
members (by ``--pbt-fitness`` over the episodes since the last round, ``--pbt-min-episodes`` at least)
take the weights of the best in one launch and explore the hyperparameters of ``--pbt-space``
(``lr:perturb:0.8,1.25:1e-6:1e-2;n_step:resample:1,3,5``):

  pbt_log.csv                  one row per replaced member: round, step, dst, src, the two
                               fitnesses and old -> new of every name of the space

Usage: python -m Louvre_Evacuation.runners.train_pop --members 8 --envs 4096 --steps 2000 \\
           --lr 1e-3,3e-4,1e-4,3e-5,1e-3,3e-4,1e-4,3e-5 --gamma 0.99   (from dqn-marl_amd/)
"""
import argparse
import csv
import json
import math
import os
import sys

project_root = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if project_root not in sys.path:
    sys.path.insert(0, project_root)

import torch  # noqa: E402
import yaml  # noqa: E402

PBT_COLUMNS = ["round", "step", "dst", "src", "fitness_dst", "fitness_src"]  # then <name>_old, <name>_new per name
CSV_COLUMNS = ["step", "episodes", "reward", "evac_rate", "death_rate", "length", "loss", "epsilon"]
SUMMARY_KEYS = ("reward", "evac_rate", "death_rate")
SUMMARY_COLUMNS = ["step"] + [f"{k}_{s}" for k in SUMMARY_KEYS for s in ("mean", "std", "min", "max")] + ["best_member"]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", default=os.path.join(project_root, "configs", "dqn.yaml"))
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--envs", type=int, default=4096, help="envs over all members (a multiple of --members)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--log-every", type=int, default=100)
    ap.add_argument("--out", default=None, help="output directory (default: the config's save_path)")
    ap.add_argument("--batch", type=int, default=None, help="learn batch per member (default: max(256, batch_size))")
    ap.add_argument("--seed", type=int, default=0, help="dropout / exploration / replay draws; seeds default to seed + k")
    for flag, what in (("--lr", "learning rate"), ("--gamma", "discount"), ("--epsilon-decay", "epsilon decay"),
                       ("--target-every", "learn steps between target copies"), ("--seeds", "initial-weight seed")):
        ap.add_argument(flag, default=None, metavar="a,b,..", help=f"{what}: one value, or one per member")
    ap.add_argument("--double-q", action="store_true", default=None,
                    help="Double-Q targets for every member (config: agent.double_dqn)")
    for flag, what in (("--loss", "TD loss, mse or huber (config: agent.loss; mse)"),
                       ("--huber-delta", "Huber delta (config: agent.huber_delta; 1.0)"),
                       ("--target-tau", "soft target rate per learn step, 0: the hard copy (config: agent.target_tau)"),
                       ("--n-step", "n-step returns from the member's ring, 1..32 (config: agent.n_step; 1)")):
        ap.add_argument(flag, default=None, metavar="a,b,..", help=f"{what}: one value, or one per member")
    ap.add_argument("--eval-episodes", type=int, default=0, help="episodes per env of a final greedy evaluation")
    ap.add_argument("--eval-envs", type=int, default=None, help="envs of that evaluation (default: a member's envs)")
    ap.add_argument("--pbt-every", type=int, default=0,
                    help="steps between exploit / explore rounds, a multiple of --log-every (0: no rounds)")
    ap.add_argument("--pbt-frac", type=float, default=0.25, help="share of the members replaced per round")
    ap.add_argument("--pbt-min-episodes", type=int, default=1,
                    help="episodes a member must have finished since the last round to take part in one")
    ap.add_argument("--pbt-fitness", default="return_mean", choices=["return_mean", "evac_rate", "neg_death_rate"])
    ap.add_argument("--pbt-space", default="lr:perturb:0.8,1.25:1e-6:1e-2", metavar="name:spec;..",
                    help="what a receiver explores: name:perturb:factors:lo:hi or name:resample:values, joined by ';'")
    return ap.parse_args(argv)


def pbt_scheduler(args, people: int):
    """The scheduler the --pbt-* flags ask for, or None with --pbt-every 0 (ValueError naming the flag;
    no device needed)."""
    if args.pbt_every == 0:
        return None
    if args.pbt_every < 0 or args.pbt_every % args.log_every:
        raise ValueError(f"--pbt-every must be a positive multiple of --log-every = {args.log_every}, "
                         f"not {args.pbt_every}")
    from evacx.pbt import PBTScheduler, parse_space
    return PBTScheduler(args.members, parse_space(args.pbt_space), frac=args.pbt_frac,
                        min_episodes=args.pbt_min_episodes, fitness=args.pbt_fitness, seed=args.seed, people=people)


def pbt_rows(round_: int, step: int, decisions, names) -> list:
    """The pbt_log.csv rows of one round's decisions."""
    return [[round_, step, d["dst"], d["src"], repr(d["fitness_dst"]), repr(d["fitness_src"])] +
            [x if isinstance(x, str) else repr(x) for n in names for x in (d["old"][n], d["new"][n])]
            for d in decisions]


def broadcast(name: str, text, K: int, conv, default):
    """A comma-separated option as K values: one value is given to every member, K values one each;
    None: the default for every member. ValueError naming the option otherwise (no device needed)."""
    if text is None:
        return [default] * K
    parts = [p.strip() for p in str(text).split(",")]
    try:
        vals = [conv(p) for p in parts]
    except ValueError:
        raise ValueError(f"--{name}: cannot read {text!r} as {conv.__name__} values") from None
    if len(vals) == 1:
        return vals * K
    if len(vals) != K:
        raise ValueError(f"--{name}: {len(vals)} values for {K} members (give one, or one per member): {text!r}")
    return vals


def member_hparams(args, agent_cfg) -> dict:
    """The per-member lists the trainer takes, from the flags and the config's agent section."""
    K = args.members
    return dict(lr=broadcast("lr", args.lr, K, float, float(agent_cfg.get("learning_rate", 1e-4))),
                gamma=broadcast("gamma", args.gamma, K, float, float(agent_cfg.get("gamma", 0.99))),
                epsilon_decay=broadcast("epsilon-decay", args.epsilon_decay, K, float,
                                        float(agent_cfg.get("epsilon_decay", 0.9995))),
                target_every=broadcast("target-every", args.target_every, K, int,
                                       int(agent_cfg.get("target_update_freq", 200))),
                init_seeds=[args.seed + k for k in range(K)] if args.seeds is None else
                broadcast("seeds", args.seeds, K, int, 0))


def member_options(args, agent_cfg) -> dict:
    """The learner options the trainer takes: double_q (one bool), and loss, huber_delta, target_tau
    and n_step as per-member lists, from the flags and the optional agent keys train_vec reads
    (double_dqn, loss, huber_delta, target_tau, n_step). The values are checked as the trainer's."""
    from evacx.population import per_member
    K = args.members
    o = dict(loss=broadcast("loss", args.loss, K, str, str(agent_cfg.get("loss", "mse"))),
             huber_delta=broadcast("huber-delta", args.huber_delta, K, float, float(agent_cfg.get("huber_delta", 1.0))),
             target_tau=broadcast("target-tau", args.target_tau, K, float, float(agent_cfg.get("target_tau", 0.0))),
             n_step=broadcast("n-step", args.n_step, K, int, agent_cfg.get("n_step", 1)))
    for name, v in o.items():
        per_member(name, v, K)
    o["double_q"] = bool(args.double_q if args.double_q is not None else agent_cfg.get("double_dqn", False))
    return o


def rank_key(row):
    """overnight_experiments.py's ordering: lowest death rate, then highest evacuation rate; a member
    without a finished episode goes last."""
    if row["episodes"] < 1:
        return (1, 0.0, 0.0)
    return (0, row["death_rate"], -row["evac_rate"])


def summary_row(step: int, rows) -> list:
    """One population_summary.csv row from the members' episode rows (None: no episode yet)."""
    out = [step]
    for key in ("return_mean", "evac_rate", "death_rate"):
        vals = [r[key] for r in rows if r[key] is not None]
        if not vals:
            out += [""] * 4
            continue
        mean = sum(vals) / len(vals)
        std = math.sqrt(max(sum(v * v for v in vals) / len(vals) - mean * mean, 0.0))
        out += [repr(mean), repr(std), repr(min(vals)), repr(max(vals))]
    return out + [min(range(len(rows)), key=lambda k: rank_key(rows[k]))]


def _fmt(v, spec):
    return "n/a" if v is None else format(v, spec)


def train_pop(args):
    from evacx.env import DeviceLayout
    from evacx.layout import LayoutSpec, build_tables
    from evacx.population import PopulationTrainer
    K = args.members
    if args.steps < 1 or args.log_every < 1:
        raise ValueError("--steps and --log-every must be >= 1")
    with open(args.config, "r", encoding="utf-8") as f:
        config = yaml.safe_load(f)
    ec, ac = config["env"], config["agent"]
    hp = member_hparams(args, ac)
    opts = member_options(args, ac)
    sched = pbt_scheduler(args, int(ec["num_people"]))
    if not torch.cuda.is_available():
        raise RuntimeError("train_pop needs an MI355X (HIP) device; no CPU fallback exists")
    out_dir = args.out or os.path.join(project_root, config.get("save_path", "dqn_results"))
    ex = ec.get("exit_location", [36, 15])
    spec = LayoutSpec(L=int(ec["width"]), W=int(ec["height"]), exit=(int(ex[0]), int(ex[1])))
    device = torch.device("cuda", torch.cuda.current_device())
    lay = DeviceLayout(build_tables(spec), int(ec["num_people"]), device=device)
    batch = args.batch or max(256, int(ac.get("batch_size", 32)))
    n = (args.envs // max(K, 1)) * lay.R  # a member's rows per push
    # at least two pushes in the ring, and a whole chain of the deepest member's n_step of them
    capacity = max(int(ac.get("memory_size", 50000)), 4 * batch, max(2, max(opts["n_step"])) * n)
    tr = PopulationTrainer(lay, args.envs, members=K, seed=args.seed, batch=batch, replay_capacity=capacity,
                           epsilon=float(ac.get("epsilon", 1.0)), epsilon_min=float(ac.get("epsilon_min", 0.02)),
                           episode_stats=True, **hp, **opts)
    dirs = [os.path.join(out_dir, f"member{k}") for k in range(K)]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    print(f"env {spec.L}x{spec.W}, {lay.P} people; {K} members x {args.envs // K} envs, batch {batch} and replay "
          f"{capacity} per member on {device}; lr {hp['lr']}, gamma {hp['gamma']}, epsilon decay "
          f"{hp['epsilon_decay']}, target every {hp['target_every']}, seeds {hp['init_seeds']}; "
          f"{'double-Q' if opts['double_q'] else 'max'} target, loss {opts['loss']}, huber delta {opts['huber_delta']}, "
          f"target tau {opts['target_tau']}, n_step {opts['n_step']}")
    files = [open(os.path.join(d, "training_log.csv"), "w", newline="") for d in dirs]
    rows = None
    if sched is not None:
        names = sorted(sched.space)
        files.append(open(os.path.join(out_dir, "pbt_log.csv"), "w", newline=""))
        plog = csv.writer(files[-1])
        plog.writerow(PBT_COLUMNS + [f"{n}_{s}" for n in names for s in ("old", "new")])
        files[-1].flush()
    try:
        logs = [csv.writer(f) for f in files[:K]]  # (files[K], with a scheduler: pbt_log.csv)
        for log in logs:
            log.writerow(CSV_COLUMNS)
        with open(os.path.join(out_dir, "population_summary.csv"), "w", newline="") as sf:
            slog = csv.writer(sf)
            slog.writerow(SUMMARY_COLUMNS)
            for step in range(1, args.steps + 1):
                tr.step()
                if step % args.log_every and step != args.steps:
                    continue
                summary = tr.episode_summary()  # the only host sync of the loop
                rows = summary["per_member"]
                loss = None if tr.last_loss is None else tr.last_loss.tolist()
                for k, (log, s) in enumerate(zip(logs, rows)):
                    log.writerow([step, s["episodes"]] + ["" if v is None else repr(v) for v in
                                 (s["return_mean"], s["evac_rate"], s["death_rate"], s["length_mean"],
                                  None if loss is None else loss[k])] + [repr(float(tr.epsilon[k]))])
                    files[k].flush()
                srow = summary_row(step, rows)
                slog.writerow(srow)
                sf.flush()
                done = [s for s in rows if s["episodes"] >= 1]
                print(f"step {step:7d}: episodes={sum(s['episodes'] for s in rows):6d}, death rate "
                      f"{_fmt(min((s['death_rate'] for s in done), default=None), '.2%')} .. "
                      f"{_fmt(max((s['death_rate'] for s in done), default=None), '.2%')}, best member {srow[-1]}")
                if sched is None:
                    continue
                sched.observe(summary)
                if step % args.pbt_every == 0:
                    rnd = sched.round
                    decisions = sched.round_(tr)
                    plog.writerows(pbt_rows(rnd, step, decisions, names))
                    files[-1].flush()
                    print(f"pbt round {rnd} at step {step}: " + (", ".join(
                        f"{d['dst']} <- {d['src']} (" + ", ".join(f"{n} {d['old'][n]!r} -> {d['new'][n]!r}" for n in names)
                        + ")" for d in decisions) or "no member replaced"))
    finally:
        for f in files:
            f.close()
    tr.sync()
    tr.env.check_err()
    for k, d in enumerate(dirs):
        torch.save(tr.checkpoint(k), os.path.join(d, "dqn_model.pth"))
    best = min(range(K), key=lambda k: rank_key(rows[k]))
    with open(os.path.join(out_dir, "best_member.json"), "w") as f:
        json.dump(dict(member=best, episodes=rows[best]["episodes"], death_rate=rows[best]["death_rate"],
                       evac_rate=rows[best]["evac_rate"], reward=rows[best]["return_mean"], lr=tr.lr[best],
                       gamma=tr.gamma[best], epsilon_decay=tr.epsilon_decay[best],
                       target_every=tr.target_every[best], seed=tr.init_seeds[best],
                       model=os.path.join(f"member{best}", "dqn_model.pth")), f, indent=2)
    print(f"best member {best}; results in {out_dir}")
    if args.eval_episodes > 0:
        from evacx.evaluate import evaluate
        envs = args.eval_envs or args.envs // K
        for k in range(K):
            ev = evaluate(lay, envs, args.eval_episodes, "greedy", learner=tr.member_learner(k), seed=args.seed)
            print(f"member {k}: greedy evaluation over {ev['episodes']} episodes: reward={ev['return_mean']:.2f}, "
                  f"evac={ev['evac_rate']:.2%}, death={ev['death_rate']:.2%}, len={ev['length_mean']:.1f}")
    return tr


def main(argv=None):
    try:
        return train_pop(parse_args(argv))
    except KeyboardInterrupt:
        print("training interrupted")


if __name__ == "__main__":
    main()
