"""`python -m dronerl_amd.per_train`: `dronerl_amd.train` with prioritized
replay implied, for every net family one agent trains on: dense nets of
widths up to 128 (dqn.PrioritizedDQNLearner), dense nets up to 256 wide
(--hidden_layers 256 128 64: dqn.PrioritizedWideDQNLearner) and conv nets
(--network_type conv: dqn.PrioritizedConvDQNLearner).

The command line is train's; --per_alpha, --per_beta, --per_beta_steps
(default: num_steps) and --per_eps give PrioritizedReplay's keywords, with
train's range checks.  --use_sharding is refused by name: the priority tree
covers one GPU's ring.  Output, checkpoints and the final eval are
`train.main`'s (train.run).
"""
from __future__ import annotations

SHARDING_REFUSAL = ("per_train with --use_sharding is not implemented: the priority tree covers one GPU's ring "
                    "(python -m dronerl_amd.train --use_sharding draws uniformly)")


def parse_args(argv=None):
    """train.parse_args with prioritized replay on for dense, wide and conv
    nets alike (train's own --prioritized_replay keeps its refusals: the flag
    is taken out before train parses the rest)."""
    import argparse

    from .train import parse_args as train_args
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--prioritized_replay", action="store_true", default=True)  # (implied)
    ap.add_argument("--use_sharding", action="store_true", default=False)
    own, rest = ap.parse_known_args(argv)
    if own.use_sharding:
        raise ValueError(SHARDING_REFUSAL)
    args = train_args(rest)  # (--per_beta_steps filled from num_steps)
    if args.per_alpha < 0 or not 0 <= args.per_beta <= 1 or args.per_beta_steps < 0 or args.per_eps < 0:
        raise ValueError("--per_alpha and --per_eps must be >= 0, --per_beta in [0, 1], --per_beta_steps >= 0")
    args.prioritized_replay = True
    return args


def main(argv=None) -> dict:
    """Train with prioritized replay, save, evaluate: train.main's output."""
    from .train import run
    return run(parse_args(argv))


if __name__ == "__main__":
    main()
