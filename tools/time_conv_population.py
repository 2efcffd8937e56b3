#!/usr/bin/env python3
"""Time a conv population's training step beside the single-agent train() step (HIP events).

1. For train_jax.py's default conv net (one 3x3 layer of 8 channels, padding 1) and the sweep's conv net
   (run_jax_sweep.py: conv 6->16->32 k3 p1, dense 128-64), on train_jax.py's 9x9 grid with 4 drones, 8 envs per
   agent, batch 8: population.train_population(network_type="conv") at P = 1, 8, 64 and 256 members, and beside
   it, in the same process, train.train(network_type="conv") for ONE such agent on the unchanged single-agent path
   -- the yardstick (never the population at P = 1).  Both loops time themselves with events around their steps
   (setup outside).  Each figure is the median of --reps repetitions of --iters steps, the variants alternating
   inside a repetition; the spread is the repetitions' min..max.  Reported: the step's time, aggregate agent-steps
   per second, the time P serial train() runs would take for the same steps, and the smallest measured P at which
   the population wins beyond both spreads.
2. --trace-workload runs only one population loop (P = 64, the sweep's conv net, 210 steps): the workload of a
   `rocprofv3 --kernel-trace --stats` run of its own, whose kernel_stats CSV a later call records with
   --stats-csv (the per-launch split of one step).

Writes one JSON file with the command line in the record.  bench.py does not time this path.
"""
import argparse
import csv
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def _c(out_channels):
    return {"out_channels": out_channels, "kernel_size": 3, "stride": 1, "padding": 1}


# name -> (conv layers, dense widths)
NETS = {"train_jax_default_8": ((_c(8),), ()), "sweep_16_32_d128_64": ((_c(16), _c(32)), (128, 64))}
TRACE_NET = "sweep_16_32_d128_64"
MEMBERS = (1, 8, 64, 256)
ENVS, BATCH, RING = 8, 8, 4096


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
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--stats-csv", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV to record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_population", "population.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    ep = EnvParams(n_drones=4, grid_size=9, window_radius=3)
    if args.stats_csv:
        with open(args.out) as f:
            result = json.load(f)
        with open(args.stats_csv) as f:
            rows = [r for r in csv.DictReader(f) if "drl_" in (r.get("Name") or "")]
        result["kernel_trace"] = {"command": "rocprofv3 --kernel-trace --stats -- python tools/time_conv_population.py "
                                             "--trace-workload", "net": TRACE_NET, "members": 64, "steps": 210,
                                  "kernels": rows}
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({"wrote": args.out, "kernels": len(rows)}))
        return

    def pop_step_us(net, P, steps):
        conv, dense = net
        hp = DQNHParams(batch=BATCH, num_steps=steps)
        r = train_population(ep, [hp] * P, ENVS, steps, memory_size=RING, seeds=list(range(P)), network_type="conv",
                             conv_layers=conv, conv_dense_layers=dense)
        return P / r.agent_steps_per_s * 1e6

    def single_step_us(net, steps):
        conv, dense = net
        r = train(ep, ENVS, steps, hp=DQNHParams(batch=BATCH, num_steps=steps), memory_size=RING, network_type="conv",
                  conv_layers=conv, conv_dense_layers=dense)
        return ENVS / r.env_steps_per_s * 1e6

    if args.trace_workload:
        pop_step_us(NETS[TRACE_NET], 64, 210)
        print(json.dumps({"net": TRACE_NET, "members": 64, "steps": 210}))
        return
    # (the command as it measures: where the record is written is not part of it)
    argv = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and not a.startswith("--out=")
            and (i == 0 or sys.argv[i] != "--out")]
    result = {"command": " ".join(["python", "tools/time_conv_population.py", *argv]), "iters": args.iters,
              "reps": args.reps, "device": torch.cuda.get_device_name(0), "envs_per_agent": ENVS, "batch": BATCH,
              "ring_slots": RING, "env": "9x9, 4 drones, radius 3", "nets": {}}
    for name, net in NETS.items():
        variants = {"train_single_agent": lambda: single_step_us(net, args.iters)}
        for P in MEMBERS:
            variants[f"population_P{P}"] = lambda P=P: pop_step_us(net, P, args.iters)
        for k in variants:  # (warm-up: the first launches load the kernels)
            if k == "train_single_agent":
                single_step_us(net, 20)
            else:
                pop_step_us(net, int(k.split("P")[-1]), 20)
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                times[k].append(fn())
        r = {k: summary(v) for k, v in times.items()}
        one = r["train_single_agent"]
        crossover = None
        for P in MEMBERS:
            s = r[f"population_P{P}"]
            s["agent_steps_per_s"] = P / s["median_us"] * 1e6
            s["serial_train_runs_us"] = P * one["median_us"]
            s["speedup_over_serial"] = P * one["median_us"] / s["median_us"]
            # beaten by more than both spreads (the serial runs' spread is P times one run's)
            s["beats_serial_beyond_spreads"] = bool(s["max_us"] + 0.0 < P * one["min_us"])
            if crossover is None and s["beats_serial_beyond_spreads"]:
                crossover = P
        one["agent_steps_per_s"] = 1e6 / one["median_us"]
        r["smallest_measured_P_that_beats_serial"] = crossover
        result["nets"][name] = r
        print(f"{name}: train() {one['median_us']:.1f} us/step ({one['min_us']:.1f}..{one['max_us']:.1f}); " + "; ".join(
            f"P={P} {r[f'population_P{P}']['median_us']:.1f} us ({r[f'population_P{P}']['min_us']:.1f}.."
            f"{r[f'population_P{P}']['max_us']:.1f}), x{r[f'population_P{P}']['speedup_over_serial']:.1f}"
            for P in MEMBERS) + f"; crossover P={crossover}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
