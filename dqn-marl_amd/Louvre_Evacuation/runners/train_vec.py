"""Vectorised DQN training with episode logging: evacx.trainer.VecTrainer over many envs.

Reads the env and agent sections of ``configs/dqn.yaml`` (the file the single-env runner
reads), trains ``--envs`` copies of that env for ``--steps`` vectorised steps with the
device-resident trainer, and every ``--log-every`` steps takes one ``episode_summary()``
of the episodes finished since the last one: a printed line, a CSV row
(``training_log.csv``: step, episodes, reward, evac_rate, death_rate, length, loss,
epsilon) and ``best_model.pth`` whenever the window's mean return beats the best so
far; ``dqn_model.pth`` at the end. Checkpoints are the reference's dict (q_network,
target_network, optimizer, epsilon, steps: agents/dqn_agent.py:174-191), so a ``--qnet
conv`` file loads through the drop-in ``DQNAgent.load``. ``--eval-episodes N`` ends with
a greedy evaluation (evacx.evaluate) of N episodes per env.

``--double-q``, ``--loss huber`` (``--huber-delta``) and ``--target-tau`` turn on the
learner's Double-Q targets, Huber loss and soft target updates (defaults from the optional
``agent:`` keys ``double_dqn``, ``loss``, ``huber_delta``, ``target_tau`` of the config).
``--n-step N`` (default: the optional ``agent:`` key ``n_step``, else 1) trains on n-step
returns gathered from the replay ring.
``--robots R`` builds the env with R robots (``evaluate_vec.build_spec``) and ``--nets`` chooses who
learns: ``shared`` (one network for every robot, the default), ``per_robot`` (robot r its own network,
memory and optimizer) or ``qmix`` (per-robot networks under a QMIX mixer); the last two need
``--robots >= 2`` and ``--qnet mlp``, take the same option flags, and write ``agent<r>.pth`` per robot
(the reference's dict; ``evaluate_vec --per-robot / --qmix`` loads them) and, for QMIX, ``mixer.pth``;
the best window's copies are ``best_agent<r>.pth`` and ``best_mixer.pth``.
``--learn-stats`` turns on the learner diagnostics: at every log line one more
line and a row of ``learn_log.csv`` with the window's Q / target / TD-error statistics, gradient
norm and clipping, non-finite counts, and the value probe's bias, RMSE and correlation.

Usage: python -m Louvre_Evacuation.runners.train_vec --envs 4096 --steps 2000   (from dqn-marl_amd/)
"""
import argparse
import csv
import os
import sys
from collections import OrderedDict

project_root = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if project_root not in sys.path:
    sys.path.insert(0, project_root)

import torch  # noqa: E402
import yaml  # noqa: E402

CSV_COLUMNS = ["step", "episodes", "reward", "evac_rate", "death_rate", "length", "loss", "epsilon"]
# learn_log.csv (--learn-stats): the learn statistics' window, then the value probe's
LEARN_COLUMNS = ["step", "learn_steps", "q_mean", "qmax_mean", "target_mean", "td_abs_mean", "td_rms", "td_p50",
                 "td_p90", "td_p99", "td_abs_max", "greedy_frac", "grad_norm_mean", "grad_norm_max", "clipped_frac",
                 "rows_bad", "steps_bad", "probes", "q0_mean", "return_mean", "bias", "rmse", "corr"]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", default=os.path.join(project_root, "configs", "dqn.yaml"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--log-every", type=int, default=100)
    ap.add_argument("--qnet", choices=["mlp", "conv"], default="mlp")
    ap.add_argument("--robots", type=int, default=1, help="robots per env (1: EvacuationEnv; 2: EvacuationEnvMulti)")
    ap.add_argument("--nets", choices=["shared", "per_robot", "qmix"], default="shared",
                    help="one Q-network for every robot, one per robot, or one per robot under a QMIX mixer")
    ap.add_argument("--out", default=None, help="output directory (default: the config's save_path)")
    ap.add_argument("--eval-episodes", type=int, default=0, help="episodes per env of a final greedy evaluation")
    ap.add_argument("--eval-envs", type=int, default=None, help="envs of that evaluation (default: --envs)")
    ap.add_argument("--batch", type=int, default=None, help="learn batch (default: max(256, the config's batch_size))")
    ap.add_argument("--seed", type=int, default=0)
    # defaults of the next four: the config's optional agent keys (td_options), else off
    ap.add_argument("--double-q", action=argparse.BooleanOptionalAction, default=None,
                    help="Double-Q targets (config: agent.double_dqn)")
    ap.add_argument("--loss", choices=["mse", "huber"], default=None, help="TD loss (config: agent.loss; mse)")
    ap.add_argument("--huber-delta", type=float, default=None, help="config: agent.huber_delta; 1.0")
    ap.add_argument("--target-tau", type=float, default=None,
                    help="soft target update rate per learn step; 0: the periodic hard copy (config: agent.target_tau)")
    ap.add_argument("--n-step", type=int, default=None,
                    help="n-step returns from the replay ring, 1..32 (config: agent.n_step; 1: one-step targets)")
    ap.add_argument("--learn-stats", action="store_true",
                    help="learner diagnostics on the device: learn-batch statistics and the value probe "
                         "(learn_log.csv)")
    return ap.parse_args(argv)


def td_options(args, agent_cfg) -> dict:
    """The learner's options: a flag given on the command line, else the config's optional
    agent key, else off. Validated here (no device needed)."""
    from evacx.qnet import validate_td_options

    def pick(flag, key, default):
        return flag if flag is not None else agent_cfg.get(key, default)
    o = dict(double_q=bool(pick(args.double_q, "double_dqn", False)), loss=str(pick(args.loss, "loss", "mse")),
             huber_delta=float(pick(args.huber_delta, "huber_delta", 1.0)),
             target_tau=float(pick(args.target_tau, "target_tau", 0.0)))
    validate_td_options(o["loss"], o["huber_delta"], o["target_tau"])
    return o


def n_step_option(args, agent_cfg) -> int:
    """--n-step, else the config's optional agent key n_step, else 1 (no device needed)."""
    from evacx._lib import NSTEP_MAX
    n = args.n_step if args.n_step is not None else agent_cfg.get("n_step", 1)
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= NSTEP_MAX:
        raise ValueError(f"n_step must be an integer in [1, {NSTEP_MAX}], not {n!r}")
    return n


def nets_option(args) -> str:
    """--nets checked against --robots, --qnet and --learn-stats (no device needed)."""
    if isinstance(args.robots, bool) or not isinstance(args.robots, int) or args.robots < 1:
        raise ValueError(f"--robots must be an integer >= 1, not {args.robots!r}")
    if args.nets != "shared":
        if args.robots < 2:
            raise ValueError(f"--nets {args.nets} needs --robots >= 2 (one network per robot), not {args.robots}")
        if args.qnet != "mlp":
            raise ValueError(f"--nets {args.nets} needs --qnet mlp: the grouped kernels run the MLP")
    if args.nets == "qmix" and args.learn_stats:
        raise ValueError("--learn-stats needs --nets shared or per_robot: the QMIX target is the mixer's")
    return args.nets


def batch_and_capacity(batch: int, memory_size: int, envs: int, R: int, n_step: int, nets: str):
    """(learn batch, replay capacity) of a run (no device needed). The ring is a power of two that
    holds the config's memory_size, four batches, at least two pushes and a whole chain of n_step of
    them. Per-robot and QMIX nets learn on batch / R rows per net and own the ring slots == robot
    (mod R): the batch goes up to a multiple of 2 R and the capacity to a multiple of R (any robot
    count, not only the powers of two)."""
    if nets != "shared":
        batch = -(-batch // (2 * R)) * 2 * R
    capacity = 1 << max(10, (max(memory_size, 4 * batch, max(2, n_step) * envs * R) - 1).bit_length())
    if nets != "shared":
        capacity = -(-capacity // R) * R
    return batch, capacity


def agent_checkpoint(tr, g: int) -> dict:
    """The reference's checkpoint dict of robot g's network (nets "per_robot" / "qmix")."""
    from types import SimpleNamespace

    from Louvre_Evacuation.agents.dqn_agent import _AdamView
    gl = tr.glearner
    view = SimpleNamespace(lr=gl.lr, betas=gl.betas, eps=gl.eps, shapes=gl.shapes, adam_step=gl.adam_step, m=gl.m[g],
                           v=gl.v[g])
    return {"q_network": OrderedDict((k, v.detach().cpu().clone()) for k, v in gl.state_dict(g).items()),
            "target_network": OrderedDict((k, v.detach().cpu().clone()) for k, v in gl.target[g].state_dict().items()),
            "optimizer": _AdamView(view).state_dict(),
            "epsilon": float(tr.epsilon),
            "steps": int(tr.learn_steps)}


def mixer_checkpoint(tr) -> dict:
    """mixer.pth: the QMIX mixer's state_dict and its target's (MixingNetwork's keys and shapes)."""
    qm, n = tr.qmix, tr.R

    def sd(flat):
        f = flat.detach().cpu().clone()
        return OrderedDict([("fc1_weight", f[:n * 32].view(n, 32)), ("fc1_bias", f[n * 32:n * 32 + 32]),
                            ("fc2_weight", f[n * 32 + 32:n * 32 + 64].view(32, 1)), ("fc2_bias", f[n * 32 + 64:])])
    return {"mixing_network": sd(qm.mix), "target_mixing_network": sd(qm.mix_t), "steps": int(tr.learn_steps)}


def save_checkpoints(tr, out_dir: str, shared_name: str, prefix: str = ""):
    """The shared net's dict under shared_name, or <prefix>agent<r>.pth per robot (and, for QMIX,
    <prefix>mixer.pth)."""
    if not tr.per_robot:
        torch.save(checkpoint(tr), os.path.join(out_dir, shared_name))
        return
    for g in range(tr.R):
        torch.save(agent_checkpoint(tr, g), os.path.join(out_dir, f"{prefix}agent{g}.pth"))
    if tr.qmix is not None:
        torch.save(mixer_checkpoint(tr), os.path.join(out_dir, f"{prefix}mixer.pth"))


def checkpoint(tr) -> dict:
    """The reference's checkpoint dict from the trainer's learner: plain tensors and scalars."""
    from Louvre_Evacuation.agents.dqn_agent import _AdamView
    lr = tr.learner
    return {"q_network": OrderedDict((k, v.detach().cpu().clone()) for k, v in lr.online.state_dict().items()),
            "target_network": OrderedDict((k, v.detach().cpu().clone()) for k, v in lr.target.state_dict().items()),
            "optimizer": _AdamView(lr).state_dict(),
            "epsilon": float(tr.epsilon),
            "steps": int(tr.learn_steps)}


def _fmt(v, spec):
    return "n/a" if v is None else format(v, spec)


def learn_row(step: int, learn_steps: int, ls: dict, vs: dict) -> list:
    """One learn_log.csv row (LEARN_COLUMNS) from learn_summary() and value_summary(); None: empty."""
    vals = [ls[k] for k in LEARN_COLUMNS[2:15]] + [ls["rows_bad"], ls["steps_bad"], vs["probes"]] + \
           [vs[k] for k in LEARN_COLUMNS[18:]]
    return [step, learn_steps] + ["" if v is None else repr(v) for v in vals]


def train_vec(args):
    from evacx.env import DeviceLayout
    from evacx.layout import build_tables
    from evacx.trainer import MultiAgentTrainer, VecTrainer
    from Louvre_Evacuation.runners.evaluate_vec import build_spec
    if not torch.cuda.is_available():
        raise RuntimeError("train_vec needs an MI355X (HIP) device; no CPU fallback exists")
    if args.envs < 2 or args.envs % 2 or args.steps < 1 or args.log_every < 1:
        raise ValueError("--envs must be even and >= 2, --steps and --log-every >= 1")
    nets = nets_option(args)
    with open(args.config, "r", encoding="utf-8") as f:
        config = yaml.safe_load(f)
    ec, ac = config["env"], config["agent"]
    out_dir = args.out or os.path.join(project_root, config.get("save_path", "dqn_results"))
    os.makedirs(out_dir, exist_ok=True)
    # one robot: the env of EvacuationEnv (fire_zones is stored and never read, as in the reference)
    spec = build_spec(ec, args.robots)
    device = torch.device("cuda", torch.cuda.current_device())
    lay = DeviceLayout(build_tables(spec), int(ec["num_people"]), device=device)
    opts = td_options(args, ac)
    n_step = n_step_option(args, ac)
    batch, capacity = batch_and_capacity(args.batch or max(256, int(ac.get("batch_size", 32))),
                                         int(ac.get("memory_size", 50000)), args.envs, lay.R, n_step, nets)
    # per-robot / QMIX nets take the learner options through MultiAgentTrainer
    trainer_cls = VecTrainer if nets == "shared" else MultiAgentTrainer
    tr = trainer_cls(lay, args.envs, kind=args.qnet, batch=batch, replay_capacity=capacity,
                     lr=float(ac.get("learning_rate", 1e-4)), gamma=float(ac.get("gamma", 0.99)),
                     epsilon=float(ac.get("epsilon", 1.0)), epsilon_min=float(ac.get("epsilon_min", 0.02)),
                     epsilon_decay=float(ac.get("epsilon_decay", 0.9995)),
                     target_every=int(ac.get("target_update_freq", 200)), learner_seed=args.seed,
                     act_table=lay.R % 2 == 0, episode_stats=True, n_step=n_step, learn_stats=args.learn_stats,
                     value_probe=args.learn_stats, nets=nets, **opts)
    tgt = f"soft tau {opts['target_tau']:g}" if opts["target_tau"] > 0 else f"hard copy every {tr.target_every}"
    print(f"env {spec.L}x{spec.W}, {lay.P} people, {lay.R} robots, exit {tuple(spec.exit)}; {args.envs} envs, {nets} nets, "
          f"{args.qnet} Q-network "
          f"({tr.q_arith}), batch {batch}, replay {capacity} on {device}; "
          f"{'double-Q' if opts['double_q'] else 'max'} target, "
          f"{'huber(%g)' % opts['huber_delta'] if opts['loss'] == 'huber' else 'mse'} loss, target {tgt}, "
          f"n_step {n_step}")
    best = float("-inf")
    with open(os.path.join(out_dir, "training_log.csv"), "w", newline="") as f, \
            open(os.path.join(out_dir, "learn_log.csv") if args.learn_stats else os.devnull, "w", newline="") as lf:
        log = csv.writer(f)
        log.writerow(CSV_COLUMNS)
        llog = csv.writer(lf)
        if args.learn_stats:
            llog.writerow(LEARN_COLUMNS)
        for step in range(1, args.steps + 1):
            tr.step()
            if step % args.log_every and step != args.steps:
                continue
            s = tr.episode_summary()  # the only host sync of the loop
            # (per-robot nets: one loss per robot, logged as their mean)
            loss = None if tr.last_loss is None else float(tr.last_loss.mean().item() if tr.per_robot
                                                           else tr.last_loss.item())
            log.writerow([step, s["episodes"]] + ["" if v is None else repr(v) for v in
                         (s["return_mean"], s["evac_rate"], s["death_rate"], s["length_mean"], loss)] +
                         [repr(float(tr.epsilon))])
            f.flush()
            print(f"step {step:7d}: episodes={s['episodes']:6d}, reward={_fmt(s['return_mean'], '9.2f')}, "
                  f"evac={_fmt(s['evac_rate'], '.2%')}, death={_fmt(s['death_rate'], '.2%')}, "
                  f"len={_fmt(s['length_mean'], '.1f')}, loss={_fmt(loss, '.4f')}, eps={tr.epsilon:.4f}")
            if args.learn_stats:
                ls, vs = tr.learn_summary(), tr.value_summary()
                llog.writerow(learn_row(step, tr.learn_steps, ls, vs))
                lf.flush()
                print(f"              learn: q={_fmt(ls['q_mean'], '.4g')}, target={_fmt(ls['target_mean'], '.4g')}, "
                      f"|td|={_fmt(ls['td_abs_mean'], '.4g')} (p50 {_fmt(ls['td_p50'], '.3g')}, p99 "
                      f"{_fmt(ls['td_p99'], '.3g')}, max {_fmt(ls['td_abs_max'], '.3g')}), greedy="
                      f"{_fmt(ls['greedy_frac'], '.2%')}, norm={_fmt(ls['grad_norm_mean'], '.4g')}, clipped="
                      f"{_fmt(ls['clipped_frac'], '.2%')}, bad rows/steps={ls['rows_bad']}/{ls['steps_bad']}; "
                      f"probe: n={vs['probes']}, q0={_fmt(vs['q0_mean'], '.4g')}, G={_fmt(vs['return_mean'], '.4g')}, "
                      f"bias={_fmt(vs['bias'], '.4g')}, rmse={_fmt(vs['rmse'], '.4g')}, corr={_fmt(vs['corr'], '.3f')}")
            if s["episodes"] >= 1 and s["return_mean"] > best:
                best = s["return_mean"]
                save_checkpoints(tr, out_dir, "best_model.pth", prefix="best_")
    tr.sync()
    tr.env.check_err()
    save_checkpoints(tr, out_dir, "dqn_model.pth")
    print(f"best window reward {_fmt(None if best == float('-inf') else best, '.2f')}; results in {out_dir}")
    if args.eval_episodes > 0:
        from evacx.evaluate import evaluate
        torch.cuda.current_stream(device).synchronize()
        ev = evaluate(lay, args.eval_envs or args.envs, args.eval_episodes, "greedy",
                      learner=tr.learner if not tr.per_robot else (tr.qmix or tr.glearner),
                      seed=args.seed)
        print(f"greedy evaluation over {ev['episodes']} episodes: reward={ev['return_mean']:.2f} "
              f"(std {ev['return_std']:.2f}, min {ev['return_min']:.2f}, max {ev['return_max']:.2f}), "
              f"evac={ev['evac_rate']:.2%}, death={ev['death_rate']:.2%}, len={ev['length_mean']:.1f}")
    return tr


def main(argv=None):
    try:
        return train_vec(parse_args(argv))
    except KeyboardInterrupt:
        print("training interrupted")


if __name__ == "__main__":
    main()
