"""`python -m dronerl_amd.conv_league`: a league whose learners are conv
Q-networks (league.ConvLeagueDQN; drl_convleague_act).

The command line is `dronerl_amd.league`'s (--learners, --opponents, --grid
and `dronerl_amd.train`'s options) with --conv_layers / --conv_dense_layers
for the learners' shared architecture, as `dronerl_amd.conv_sweep` takes them;
--network_type defaults to conv here, dense is refused (use
`python -m dronerl_amd.league`), and so is --use_sharding.

    python -m dronerl_amd.conv_league --learners 2 --opponents A.safetensors B.safetensors \\
        --n_drones 6 --grid_size 11 --num_envs 4096 --conv_layers '[...]' --conv_dense_layers 128 64

After training every learner is saved (checkpoint.save_conv, both formats,
with --save_final_checkpoint) and the greedy line-up is scored; the JSON line
is `dronerl_amd.league`'s.
"""
from __future__ import annotations

import json
import os

from .league import SHARDING_REFUSAL, learners_of, opponents_of

DENSE_REFUSAL = ("conv_league trains conv learners only (--network_type conv); for dense learners use "
                 "python -m dronerl_amd.league")


def parse_args(argv=None):
    """league.parse_args for conv learners.  Returns (args, points): the
    shared options (args.learners, args.opponents: the drone-index map,
    args.conv_layers, args.conv_dense_layers) and the grid's points, one per
    learner or one shared."""
    import argparse

    from .sweep import expand_grid
    from .train import parse_args as train_args
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--learners", type=int, default=2)
    ap.add_argument("--opponents", nargs="*", default=[])
    ap.add_argument("--grid", type=str, default="{}")
    ap.add_argument("--network_type", type=str, default="conv")
    ap.add_argument("--use_sharding", action="store_true", default=False)
    own, rest = ap.parse_known_args(argv)
    if own.network_type != "conv":
        raise ValueError(DENSE_REFUSAL)
    if own.use_sharding:
        raise ValueError(SHARDING_REFUSAL)
    args = train_args(["--network_type", "conv", *rest])
    if own.learners < 1:
        raise ValueError("--learners must be >= 1")
    if own.learners > args.n_drones:
        raise ValueError(f"--learners {own.learners}: more learners than drones (--n_drones {args.n_drones}); "
                         "learner k drives drone index k")
    try:
        grid = json.loads(own.grid)
    except json.JSONDecodeError as e:
        raise ValueError(f"--grid is not valid JSON: {e}")
    points = expand_grid(grid)
    from .train import refuse_double_dqn
    refuse_double_dqn(args, "the conv league (conv_league)", points)
    if len(points) not in (1, own.learners):
        raise ValueError(f"--grid has {len(points)} points: one per learner ({own.learners}) or one shared point")
    args.learners = own.learners
    args.opponents = opponents_of(own.opponents, own.learners, args.n_drones)
    return args, points


def main(argv=None) -> dict:
    """Train the conv league, save every learner, score the greedy line-up."""
    from datetime import datetime

    import torch

    from .league import evaluate_league, train_league
    from .train import env_params_of
    args, points = parse_args(argv)
    hps = learners_of(args, points)
    dev = torch.device("cuda", torch.cuda.current_device())
    K = args.learners
    res = train_league(env_params_of(args), hps, args.num_envs, args.num_steps, opponents=args.opponents,
                       reset_env_every=args.reset_env_every, memory_size=args.memory_size, seed=args.seed,
                       seeds=[args.seed + k for k in range(K)], device=dev, network_type="conv",
                       conv_layers=args.conv_layers, conv_dense_layers=tuple(args.conv_dense_layers))
    out = {"learners": K, "num_envs": args.num_envs, "num_steps": args.num_steps, "network_type": "conv",
           "conv_layers": list(args.conv_layers), "conv_dense_layers": list(args.conv_dense_layers),
           "steps_per_sec": res.agent_steps_per_s / K, "agent_steps_per_sec": res.agent_steps_per_s,
           "opponents": {str(d): p for d, p in args.opponents.items()}}
    if args.save_final_checkpoint:
        run_dir = os.path.join(args.output_dir, f"conv_league_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
        os.makedirs(run_dir, exist_ok=True)
        out["checkpoints"] = []
        for k in range(K):
            paths = {}
            for fmt in ("jax", "torch"):
                paths[fmt] = os.path.join(run_dir, f"learner_{k}_agent_{args.num_steps}_steps_{fmt}.safetensors")
                # (the metadata train_jax.py writes: its options as given)
                res.league.save(k, paths[fmt], format=fmt, conv_layers=args.conv_layers,
                                hidden_layers=tuple(args.hidden_layers))
            out["checkpoints"].append(paths)
    ev = evaluate_league(res, params=env_params_of(args, eval_env=True),
                         seeds=[args.eval_seed + i for i in range(args.num_evals)], num_steps=args.num_eval_steps,
                         device=dev, action_seed=args.eval_seed)
    out["eval"] = [{"drone": d, "role": ev["roles"][d], "reward_mean": float(ev["mean"][d]),
                    "reward_std": float(ev["std"][d]),
                    **({"final_epsilon": res.league.counters(d)["epsilon"],
                        "train_steps": res.league.counters(d)["count"]} if d < K else {})}
                   for d in range(len(ev["roles"]))]
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
