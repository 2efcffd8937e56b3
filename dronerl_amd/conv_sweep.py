"""`python -m dronerl_amd.conv_sweep`: the conv half of a hyperparameter
sweep as one population (run_jax_sweep.py draws network_type from
['dense', 'conv']; its conv runs use conv 6->16->32 (k3 p1), dense 128-64).

The command line is `dronerl_amd.sweep`'s (--grid, --members_seeds and
`dronerl_amd.train`'s options) with --conv_layers / --conv_dense_layers for
the shared architecture; --network_type defaults to conv here, dense is
refused (use `python -m dronerl_amd.sweep`), and so is --use_sharding.

After training each member is evaluated greedily (train.evaluate on
ConvPopulationDQN.member_net) and the same JSON table as dronerl_amd.sweep's
is written; with --save_final_checkpoint every member's checkpoint is written
beside it (checkpoint.save_conv).
"""
from __future__ import annotations

import json
import os

from .sweep import expand_grid, members_of

DENSE_REFUSAL = "conv_sweep trains conv nets only (--network_type conv); for dense nets use python -m dronerl_amd.sweep"


def parse_args(argv=None):
    """train.parse_args plus --grid and --members_seeds, through
    sweep.expand_grid.  Returns (args, points)."""
    import argparse

    from .train import parse_args as train_args
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--grid", type=str, default="{}")
    ap.add_argument("--members_seeds", type=int, default=1)
    ap.add_argument("--network_type", type=str, default="conv")
    ap.add_argument("--use_sharding", action="store_true", default=False)
    own, rest = ap.parse_known_args(argv)
    if own.network_type != "conv":
        raise ValueError(DENSE_REFUSAL)
    if own.use_sharding:
        raise ValueError("a population runs on one GPU (no --use_sharding)")
    args = train_args(["--network_type", "conv", *rest])
    try:
        grid = json.loads(own.grid)
    except json.JSONDecodeError as e:
        raise ValueError(f"--grid is not valid JSON: {e}")
    if own.members_seeds < 1:
        raise ValueError("--members_seeds must be >= 1")
    args.members_seeds = own.members_seeds
    points = expand_grid(grid)
    from .train import refuse_double_dqn
    refuse_double_dqn(args, "the conv population sweep (conv_sweep)", points)
    from .population import POP_MAX_MEMBERS
    if len(points) * own.members_seeds > POP_MAX_MEMBERS:
        raise ValueError(f"the population has {len(points) * own.members_seeds} members; at most {POP_MAX_MEMBERS}")
    return args, points


def main(argv=None) -> dict:
    """Train the conv population, evaluate every member, write the table."""
    from datetime import datetime

    import torch

    from .population import train_population
    from .train import env_params_of, evaluate
    args, points = parse_args(argv)
    hps, seeds, rows = members_of(args, points)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = train_population(env_params_of(args), hps, args.num_envs, args.num_steps,
                           reset_env_every=args.reset_env_every, memory_size=args.memory_size, seed=args.seed,
                           device=dev, seeds=seeds, network_type="conv", conv_layers=args.conv_layers,
                           conv_dense_layers=tuple(args.conv_dense_layers))
    run_dir = os.path.join(args.output_dir, f"conv_sweep_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    os.makedirs(run_dir, exist_ok=True)
    table = []
    for m, (hp, row) in enumerate(zip(hps, rows)):
        c = res.pop.counters(m)
        (am, asd), _, _ = evaluate(env_params_of(args, eval_env=True), res.pop.member_net(m), args.num_evals,
                                   args.num_eval_steps, args.eval_seed, device=dev)
        entry = {"member": m, **row, "batch_size": hp.batch, "learning_rate": hp.learning_rate, "gamma": hp.gamma,
                 "tau": hp.tau, "target_update_interval": hp.target_update_interval, "epsilon_end": hp.epsilon_end,
                 "epsilon_decay": hp.decay(), "epsilon_decay_every": hp.epsilon_decay_every,
                 "eval_reward_mean": am, "eval_reward_std": asd, "final_epsilon": c["epsilon"],
                 "final_loss": c["loss"], "steps": c["step"], "train_steps": c["count"]}
        if args.save_final_checkpoint:
            for fmt in ("jax", "torch"):
                path = os.path.join(run_dir, f"member_{m}_agent_{args.num_steps}_steps_{fmt}.safetensors")
                # (the metadata train_jax.py writes: its options as given)
                res.pop.save(m, path, format=fmt, conv_layers=args.conv_layers,
                             hidden_layers=tuple(args.hidden_layers))
                entry[f"checkpoint_{fmt}"] = path
        table.append(entry)
    out = {"members": len(hps), "num_envs": args.num_envs, "num_steps": args.num_steps,
           "network_type": "conv", "conv_layers": list(args.conv_layers),
           "conv_dense_layers": list(args.conv_dense_layers), "agent_steps_per_sec": res.agent_steps_per_s,
           "table": table}
    path = os.path.join(run_dir, "sweep.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    out["table_path"] = path
    print(json.dumps({"table_path": path, "members": len(hps), "agent_steps_per_sec": res.agent_steps_per_s}),
          flush=True)
    return out


if __name__ == "__main__":
    main()
