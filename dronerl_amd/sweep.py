"""`python -m dronerl_amd.sweep`: a hyperparameter sweep as one population
(run_jax_sweep.py / torch_impl/sweep.py, whose runs go one after another).

The command line is `dronerl_amd.train`'s with:
  --grid '{"learning_rate": [1e-4, 5e-4], "batch_size": [8, 16]}'
      a JSON object of lists; the product of the lists is the population,
      every other option is shared;
  --members_seeds K
      each grid point K times, with seeds seed, seed + 1, ... (the member's
      initialisation and its replay draw);
and options that every member must share (the env, num_envs, the net, the
ring, num_steps, reset_env_every) are refused inside --grid.

After training each member is evaluated greedily (train.evaluate on
PopulationDQN.member_net) and one JSON table is written: a row per member
with its hyperparameters, eval mean and std, final epsilon and loss.  With
--save_final_checkpoint every member's checkpoint is written beside it.
"""
from __future__ import annotations

import itertools
import json
import os
from typing import List, Tuple

# what a member may own (a DQNHParams field each): train's option -> why it can differ
MEMBER_OPTIONS = ("batch_size", "learning_rate", "gamma", "tau", "target_update_interval", "epsilon_start",
                  "epsilon_decay", "epsilon_decay_half_life_fraction", "epsilon_end", "epsilon_decay_every",
                  "double_dqn")  # (double_dqn: JSON booleans; the TD rule is chosen per member in one launch chain)
# what the population shares, and why
SHARED_OPTIONS = {
    "num_envs": "one env batch of members * num_envs envs serves the population: every member owns num_envs of them",
    "num_steps": "the members step together: one launch chain per step for all of them",
    "reset_env_every": "the reset is one launch over every env",
    "memory_size": "the members' rings share one allocation, cursor and size",
    "hidden_layers": "the members' blocks share one layout: the net's architecture is the population's",
    "network_type": "a population trains dense nets only",
    "seed": "use --members_seeds to repeat each point with several seeds",
}
ENV_OPTIONS = ("n_drones", "grid_size", "window_radius", "packets_factor", "dropzones_factor", "stations_factor",
               "skyscrapers_factor", "pickup_reward", "delivery_reward", "crash_reward", "charge_reward")


def expand_grid(grid: dict) -> List[dict]:
    """The product of the grid's lists, in the keys' order (the last key
    varies fastest): one dict of overrides per point."""
    if not isinstance(grid, dict):
        raise ValueError("--grid must be a JSON object of lists")
    for k, v in grid.items():
        if k in SHARED_OPTIONS:
            raise ValueError(f"--grid: {k} must be shared by every member ({SHARED_OPTIONS[k]})")
        if k in ENV_OPTIONS:
            raise ValueError(f"--grid: {k} must be shared by every member (one env batch with one set of env "
                             "parameters serves the population)")
        if k not in MEMBER_OPTIONS:
            raise ValueError(f"--grid: {k} is not a per-member option (one of {', '.join(MEMBER_OPTIONS)})")
        if not isinstance(v, list) or not v:
            raise ValueError(f"--grid: {k} must be a non-empty list")
        if k == "double_dqn" and not all(isinstance(x, bool) for x in v):
            raise ValueError("--grid: double_dqn takes JSON booleans (true / false)")
    keys = list(grid)
    return [dict(zip(keys, vals)) for vals in itertools.product(*[grid[k] for k in keys])]


def parse_args(argv=None):
    """train.parse_args plus --grid and --members_seeds.  Returns (args,
    points): the shared options and the grid's points."""
    import argparse

    from .train import parse_args as train_args
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--grid", type=str, default="{}")
    ap.add_argument("--members_seeds", type=int, default=1)
    own, rest = ap.parse_known_args(argv)
    args = train_args(rest)
    from .train import refuse_prioritized
    refuse_prioritized(args, "the population sweep")
    try:
        grid = json.loads(own.grid)
    except json.JSONDecodeError as e:
        raise ValueError(f"--grid is not valid JSON: {e}")
    if own.members_seeds < 1:
        raise ValueError("--members_seeds must be >= 1")
    if args.network_type != "dense":
        raise ValueError("a population trains dense nets only (--network_type dense)")
    if args.use_sharding:
        raise ValueError("a population runs on one GPU (no --use_sharding)")
    args.members_seeds = own.members_seeds
    points = expand_grid(grid)
    from .population import POP_MAX_MEMBERS
    if len(points) * own.members_seeds > POP_MAX_MEMBERS:
        raise ValueError(f"the population has {len(points) * own.members_seeds} members; at most {POP_MAX_MEMBERS}")
    return args, points


def members_of(args, points) -> Tuple[list, list, list]:
    """(hyperparameters, seeds, rows): a DQNHParams, a seed and the table's
    row of overrides per member -- each point members_seeds times."""
    import copy

    from .train import hparams_of
    hps, seeds, rows = [], [], []
    for pt in points:
        for k in range(args.members_seeds):
            a = copy.copy(args)
            for key, v in pt.items():
                setattr(a, key, type(getattr(args, key))(v) if getattr(args, key) is not None else v)
            a.seed = args.seed + k
            hps.append(hparams_of(a))
            seeds.append(a.seed)
            rows.append({**pt, "seed": a.seed})
    return hps, seeds, rows


def main(argv=None) -> dict:
    """Train the population, evaluate every member, write the table."""
    from datetime import datetime

    import torch

    from .population import train_population
    from .train import env_params_of, evaluate
    args, points = parse_args(argv)
    hps, seeds, rows = members_of(args, points)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = train_population(env_params_of(args), hps, args.num_envs, args.num_steps, hidden=tuple(args.hidden_layers),
                           reset_env_every=args.reset_env_every, memory_size=args.memory_size, seed=args.seed,
                           device=dev, seeds=seeds)
    run_dir = os.path.join(args.output_dir, f"sweep_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    os.makedirs(run_dir, exist_ok=True)
    table = []
    for m, (hp, row) in enumerate(zip(hps, rows)):
        c = res.pop.counters(m)
        (am, asd), _, _ = evaluate(env_params_of(args, eval_env=True), res.pop.member_net(m), args.num_evals,
                                   args.num_eval_steps, args.eval_seed, device=dev)
        entry = {"member": m, **row, "batch_size": hp.batch, "learning_rate": hp.learning_rate, "gamma": hp.gamma,
                 "tau": hp.tau, "target_update_interval": hp.target_update_interval, "epsilon_end": hp.epsilon_end,
                 "epsilon_decay": hp.decay(), "epsilon_decay_every": hp.epsilon_decay_every,
                 "double_dqn": bool(hp.double_dqn),
                 "eval_reward_mean": am, "eval_reward_std": asd, "final_epsilon": c["epsilon"],
                 "final_loss": c["loss"], "steps": c["step"], "train_steps": c["count"]}
        if args.save_final_checkpoint:
            for fmt in ("jax", "torch"):
                path = os.path.join(run_dir, f"member_{m}_agent_{args.num_steps}_steps_{fmt}.safetensors")
                res.pop.save(m, path, format=fmt)
                entry[f"checkpoint_{fmt}"] = path
        table.append(entry)
    out = {"members": len(hps), "num_envs": args.num_envs, "num_steps": args.num_steps,
           "hidden_layers": list(args.hidden_layers), "agent_steps_per_sec": res.agent_steps_per_s, "table": table}
    path = os.path.join(run_dir, "sweep.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    out["table_path"] = path
    print(json.dumps({"table_path": path, "members": len(hps), "agent_steps_per_sec": res.agent_steps_per_s}),
          flush=True)
    return out


if __name__ == "__main__":
    main()
