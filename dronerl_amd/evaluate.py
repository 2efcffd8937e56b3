"""Score submissions as the reference evaluator does (evaluate_agent.py's call shape):

    python -m dronerl_amd.evaluate MODEL [MODEL ...] [--baselines DIR] [--episodes N] [--steps N]

Every MODEL (.safetensors) meets the five baselines of DIR (dqn-agent-1..5.safetensors; default
./sample_models) over the evaluator's first N seeded episodes, all models in one batch of envs on the GPU
(dronerl_amd.evaluator.evaluate_submissions).  One JSON line per model: score / score_secondary are the mean and
standard deviation over episodes of the submission's summed rewards, "scores" the [episodes][agents] table.
"""
import argparse
import json

from .evaluator import EPISODE_SEEDS, TOTAL_EPISODE_STEPS, evaluate_submissions


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m dronerl_amd.evaluate", description=__doc__.split("\n")[0])
    ap.add_argument("model_paths", nargs="+", metavar="MODEL", help="model file(s) (.safetensors)")
    ap.add_argument("--baselines", default="sample_models", metavar="DIR",
                    help="directory of dqn-agent-1..5.safetensors (default: sample_models)")
    ap.add_argument("--episodes", type=int, default=len(EPISODE_SEEDS), metavar="N",
                    help=f"the evaluator's first N episode seeds (1..{len(EPISODE_SEEDS)})")
    ap.add_argument("--steps", type=int, default=TOTAL_EPISODE_STEPS, metavar="N", help="steps per episode")
    args = ap.parse_args(argv)
    if not 1 <= args.episodes <= len(EPISODE_SEEDS):
        ap.error(f"--episodes must lie in [1, {len(EPISODE_SEEDS)}]")
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    results = evaluate_submissions(args.model_paths, baselines=args.baselines, seeds=EPISODE_SEEDS[:args.episodes],
                                   num_steps=args.steps)
    for r in results:
        print(json.dumps({"model": r["path"], "score": r["score"], "score_secondary": r["score_secondary"],
                          "episodes": args.episodes, "steps": args.steps, "scores": r["scores"].tolist()}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
