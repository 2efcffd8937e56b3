#!/usr/bin/env python3
"""Time the prioritized population's training step (HIP events) beside its two yardsticks, in one process.

For the nets 128-64 and 256-128-64 and the batches 8 and 256 (train_jax.py's 9x9 grid with 4 drones, 8 envs per
member, a 100,000-slot ring), each a loop that times its own steps with events (setup outside):
  * population.train_population(per=...) at P = 1, 8, 64 and 256 members (alpha 0.6, beta 0.4 annealed);
  * train_population on the unchanged uniform path (drl_pop_train) at the same P: what priorities cost;
  * at 128-64, train.train(per=...) for ONE agent on the unchanged single-agent path (drl_dqn_per_train): P times
    that is what the population saves.
Each figure is the median of --reps repetitions of --iters steps, the variants alternating inside a repetition;
the spread is the repetitions' min..max.  Nothing is asserted.

--trace-workload P runs only one prioritized population loop (the 128-64 net, batch 8, 210 steps): the workload
of a `rocprofv3 --kernel-trace --stats` run of its own (the program after `--`), whose kernel_stats CSV shows the
launches per step.

Writes one JSON file with the command line in the record.  bench.py does not time this path.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

NETS = {"128_64": (128, 64), "256_128_64": (256, 128, 64)}
MEMBERS = (1, 8, 64, 256)
BATCHES = (8, 256)
ENVS, RING = 8, 100_000
PER = dict(alpha=0.6, beta0=0.4, eps=1e-6)


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v),
            "reps_us": v}


def main():
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.population import train_population
    from dronerl_amd.train import train
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-workload", type=int, default=0, metavar="P")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pop_per", "population.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    ep = EnvParams(n_drones=4, grid_size=9, window_radius=3)

    def pop_step_us(hidden, P, batch, steps, prioritized):
        hp = DQNHParams(batch=batch, num_steps=steps)
        per = [dict(PER, beta_steps=steps)] * P if prioritized else None
        r = train_population(ep, [hp] * P, ENVS, steps, hidden=hidden, memory_size=RING, seeds=list(range(P)), per=per)
        return P / r.agent_steps_per_s * 1e6

    def single_step_us(hidden, batch, steps):
        r = train(ep, ENVS, steps, hidden=hidden, hp=DQNHParams(batch=batch, num_steps=steps), memory_size=RING,
                  per=dict(PER, beta_steps=steps))
        return ENVS / r.env_steps_per_s * 1e6

    if args.trace_workload:
        pop_step_us(NETS["128_64"], args.trace_workload, 8, 210, True)
        print(json.dumps({"members": args.trace_workload, "steps": 210}))
        return
    # (the command as it measures: where the record is written is not part of it)
    argv = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and not a.startswith("--out=")
            and (i == 0 or sys.argv[i] != "--out")]
    result = {"command": " ".join(["python", "tools/time_pop_per.py", *argv]), "iters": args.iters, "reps": args.reps,
              "device": torch.cuda.get_device_name(0), "envs_per_member": ENVS, "ring_slots": RING,
              "env": "9x9, 4 drones, radius 3", "per": dict(PER, beta_steps="the run's steps"), "nets": {}}
    for name, hidden in NETS.items():
        result["nets"][name] = {}
        for batch in BATCHES:
            # (a member trains once its ring holds a batch: with 8 envs per member, batch 256 trains from step 31)
            variants = {}
            if max(hidden) <= 128:
                variants["train_single_agent_per"] = lambda: single_step_us(hidden, batch, args.iters)
            for P in MEMBERS:
                variants[f"per_population_P{P}"] = lambda P=P: pop_step_us(hidden, P, batch, args.iters, True)
                variants[f"uniform_population_P{P}"] = lambda P=P: pop_step_us(hidden, P, batch, args.iters, False)
            for fn in variants.values():  # (warm-up: the first launches load the kernels)
                fn()
            times = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, fn in variants.items():
                    times[k].append(fn())
            r = {k: summary(v) for k, v in times.items()}
            one = r.get("train_single_agent_per")
            for P in MEMBERS:
                s, u = r[f"per_population_P{P}"], r[f"uniform_population_P{P}"]
                s["agent_steps_per_s"] = P / s["median_us"] * 1e6
                s["added_over_uniform_us"] = s["median_us"] - u["median_us"]
                s["added_beyond_spreads"] = bool(s["min_us"] > u["max_us"])
                if one:
                    s["serial_per_train_runs_us"] = P * one["median_us"]
                    s["speedup_over_serial"] = P * one["median_us"] / s["median_us"]
            result["nets"][name][f"batch_{batch}"] = r
            print(f"{name} batch {batch}: " + (f"train(per) {one['median_us']:.1f} us/step; " if one else "") + "; ".join(
                f"P={P} per {r[f'per_population_P{P}']['median_us']:.1f} us ({r[f'per_population_P{P}']['min_us']:.1f}.."
                f"{r[f'per_population_P{P}']['max_us']:.1f}) uniform {r[f'uniform_population_P{P}']['median_us']:.1f} us "
                f"(+{r[f'per_population_P{P}']['added_over_uniform_us']:.1f})" for P in MEMBERS), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
