"""`python -m dronerl_amd.per_sweep`: a sweep over prioritized replay's own
knobs as one population (population.PrioritizedPopulationDQN: every member
owns a priority tree over its ring and its own alpha, beta0, beta_steps and
eps; the members sample, train and update priorities in one launch chain).

The command line is `dronerl_amd.sweep`'s (--grid, --members_seeds and
`dronerl_amd.train`'s options) with prioritized replay implied:
  * per_alpha, per_beta, per_beta_steps and per_eps join the per-member grid
    keys; outside the grid train's --per_alpha / --per_beta /
    --per_beta_steps (default: num_steps) / --per_eps give the shared values;
  * a member with per_alpha 0 and per_beta 0 draws uniformly over the written
    slots with weights of exactly 1: the control inside the same run;
  * --network_type conv, hidden widths a population does not take and
    --use_sharding are refused by name.

After training each member is evaluated greedily and dronerl_amd.sweep's JSON
table is written with the four PER columns added.
"""
from __future__ import annotations

import itertools
import json
import os
from typing import List, Tuple

from . import sweep

PER_OPTIONS = ("per_alpha", "per_beta", "per_beta_steps", "per_eps")
CONV_REFUSAL = ("per_sweep with --network_type conv is not implemented: a prioritized population trains dense nets "
                "only (conv populations draw uniformly: python -m dronerl_amd.conv_sweep)")
SHARDING_REFUSAL = "per_sweep with --use_sharding is not implemented: a population runs on one GPU"
WIDTH_REFUSAL = ("per_sweep: --hidden_layers must be 1 to 3 widths, multiples of 8 in [8, 256] (what a population "
                 "trains)")


def expand_grid(grid: dict) -> List[dict]:
    """sweep.expand_grid with the four PER options among the per-member keys."""
    if not isinstance(grid, dict):
        raise ValueError("--grid must be a JSON object of lists")
    sweep.expand_grid({k: v for k, v in grid.items() if k not in PER_OPTIONS})  # (its refusals, by name)
    for k in PER_OPTIONS:
        if k in grid and (not isinstance(grid[k], list) or not grid[k]):
            raise ValueError(f"--grid: {k} must be a non-empty list")
    keys = list(grid)
    return [dict(zip(keys, vals)) for vals in itertools.product(*[grid[k] for k in keys])]


def check_per(alpha, beta, beta_steps, eps):
    if alpha < 0 or not 0 <= beta <= 1 or beta_steps < 0 or eps < 0:
        raise ValueError("per_alpha and per_eps must be >= 0, per_beta in [0, 1], per_beta_steps >= 0")


def parse_args(argv=None):
    """train.parse_args plus --grid and --members_seeds.  Returns (args,
    points): the shared options and the grid's points."""
    import argparse

    from .train import parse_args as train_args
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--grid", type=str, default="{}")
    ap.add_argument("--members_seeds", type=int, default=1)
    ap.add_argument("--prioritized_replay", action="store_true", default=True)  # (implied)
    ap.add_argument("--network_type", type=str, default="dense")
    ap.add_argument("--use_sharding", action="store_true", default=False)
    own, rest = ap.parse_known_args(argv)
    if own.network_type != "dense":
        raise ValueError(CONV_REFUSAL)
    if own.use_sharding:
        raise ValueError(SHARDING_REFUSAL)
    args = train_args(rest)
    hl = tuple(args.hidden_layers)
    if not 1 <= len(hl) <= 3 or any(w < 8 or w > 256 or w % 8 for w in hl):
        raise ValueError(WIDTH_REFUSAL)
    try:
        grid = json.loads(own.grid)
    except json.JSONDecodeError as e:
        raise ValueError(f"--grid is not valid JSON: {e}")
    if own.members_seeds < 1:
        raise ValueError("--members_seeds must be >= 1")
    args.members_seeds = own.members_seeds
    args.prioritized_replay = True
    check_per(args.per_alpha, args.per_beta, args.per_beta_steps, args.per_eps)
    points = expand_grid(grid)
    from .train import refuse_double_dqn
    refuse_double_dqn(args, "the prioritized population sweep (per_sweep)", points)
    for pt in points:
        check_per(*[pt.get(k, getattr(args, k)) for k in PER_OPTIONS])
    from .population import POP_MAX_MEMBERS
    if len(points) * own.members_seeds > POP_MAX_MEMBERS:
        raise ValueError(f"the population has {len(points) * own.members_seeds} members; at most {POP_MAX_MEMBERS}")
    return args, points


def members_of(args, points) -> Tuple[list, list, list, list]:
    """(hyperparameters, seeds, rows, pers): sweep.members_of's three lists
    and each member's PER record (PrioritizedPopulationReplay's keywords)."""
    hps, seeds, rows = sweep.members_of(args, points)
    pers = []
    for row in rows:
        v = {k: type(getattr(args, k))(row.get(k, getattr(args, k))) for k in PER_OPTIONS}
        pers.append(dict(alpha=v["per_alpha"], beta0=v["per_beta"], beta_steps=v["per_beta_steps"], eps=v["per_eps"]))
    return hps, seeds, rows, pers


def main(argv=None) -> dict:
    """Train the prioritized population, evaluate every member, write the table."""
    from datetime import datetime

    import torch

    from .population import train_population
    from .train import env_params_of, evaluate
    args, points = parse_args(argv)
    hps, seeds, rows, pers = members_of(args, points)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = train_population(env_params_of(args), hps, args.num_envs, args.num_steps, hidden=tuple(args.hidden_layers),
                           reset_env_every=args.reset_env_every, memory_size=args.memory_size, seed=args.seed,
                           device=dev, seeds=seeds, per=pers)
    run_dir = os.path.join(args.output_dir, f"per_sweep_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    os.makedirs(run_dir, exist_ok=True)
    table = []
    for m, (hp, row, per) in enumerate(zip(hps, rows, pers)):
        c = res.pop.counters(m)
        (am, asd), (rm, rsd), _ = evaluate(env_params_of(args, eval_env=True), res.pop.member_net(m), args.num_evals,
                                           args.num_eval_steps, args.eval_seed, device=dev)
        entry = {"member": m, **row, "batch_size": hp.batch, "learning_rate": hp.learning_rate, "gamma": hp.gamma,
                 "tau": hp.tau, "target_update_interval": hp.target_update_interval, "epsilon_end": hp.epsilon_end,
                 "epsilon_decay": hp.decay(), "epsilon_decay_every": hp.epsilon_decay_every,
                 "per_alpha": per["alpha"], "per_beta": per["beta0"], "per_beta_steps": per["beta_steps"],
                 "per_eps": per["eps"], "eval_reward_mean": am, "eval_reward_std": asd, "random_reward_mean": rm,
                 "final_epsilon": c["epsilon"], "final_loss": c["loss"], "steps": c["step"], "train_steps": c["count"],
                 "pmax": float(res.replay.pmax(m).item())}
        if args.save_final_checkpoint:
            for fmt in ("jax", "torch"):
                path = os.path.join(run_dir, f"member_{m}_agent_{args.num_steps}_steps_{fmt}.safetensors")
                res.pop.save(m, path, format=fmt)
                entry[f"checkpoint_{fmt}"] = path
        table.append(entry)
    out = {"members": len(hps), "num_envs": args.num_envs, "num_steps": args.num_steps,
           "hidden_layers": list(args.hidden_layers), "prioritized_replay": True,
           "agent_steps_per_sec": res.agent_steps_per_s, "table": table}
    path = os.path.join(run_dir, "sweep.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    out["table_path"] = path
    print(json.dumps({"table_path": path, "members": len(hps), "agent_steps_per_sec": res.agent_steps_per_s}),
          flush=True)
    return out


if __name__ == "__main__":
    main()
