#!/usr/bin/env python3
"""Time the league (HIP events): its act against drl_pop_act, and its training step.

1. The act against its yardstick.  For the nets 128-64 and 256-128-64 on 7x7 windows, K = 6 learners and
   E = 4,096 and 65,536 envs: drl_league_act beside drl_pop_act (unchanged; members = K, envs_per_member = E) on
   the same K * E code rows, the same parameters, in the same process.  Before timing, both Q outputs are compared
   bit for bit.  Each figure is the median of --reps repetitions of --iters calls, the two alternating inside a
   repetition; the spread is the repetitions' min..max.  Beside each time: the arithmetic floor (the learner's
   order needs a separate multiply and add per product: 2 FLOP per MAC at half the 157.3 TF f32 vector peak) and
   the fraction of it reached.
2. The league step (act, opponents' acts, env step, every drone's code, add, train) at N = 6, side 11,
   E = 4,096, batch 8: K = 2 learners with 4 sample baselines as opponents, and K = 6 learners; beside them
   train.train's step for ONE such agent against random drones.  Context, not a bar: the league does work
   train() cannot do.
3. --trace-workload runs only one league loop (K = 2 with 4 opponents, 210 steps): the workload of a
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

NETS = {"128_64": (128, 64), "256_128_64": (256, 128, 64)}
K_ACT, ENVS_ACT = 6, (4096, 65536)
STEP_ENVS, BATCH, RING = 4096, 8, 65536
MODELS = os.path.join(REPO, "tests", "golden", "sample_models")
PEAK_F32_VECTOR = 157.3e12  # MI355X vector f32 peak (packed FMA): a multiply and an add per product run at half


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v),
            "reps_us": v}


def macs(hidden, D=294, A=5):
    sizes = [D, *hidden, A]
    return sum(sizes[i] * sizes[i + 1] for i in range(len(sizes) - 1))


def main():
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.evaluator import EVALUATOR_ENV_PARAMS, obs_code_all
    from dronerl_amd.league import LeagueDQN, train_league
    from dronerl_amd.population import PopulationDQN
    from dronerl_amd.train import train
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--stats-csv", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV to record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "league", "league.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    ep = EnvParams.from_torch_config(dict(EVALUATOR_ENV_PARAMS), window_radius=3)  # 6 drones, side 11, 7x7 windows
    baselines = {d: os.path.join(MODELS, f"dqn-agent-{d}.safetensors") for d in (2, 3, 4, 5)}  # (5: the conv net)
    if args.stats_csv:
        with open(args.out) as f:
            result = json.load(f)
        with open(args.stats_csv) as f:
            rows = [r for r in csv.DictReader(f) if "drl_" in (r.get("Name") or "")]
        result["kernel_trace"] = {"command": "rocprofv3 --kernel-trace --stats -- python tools/time_league.py "
                                             "--trace-workload", "learners": 2, "opponents": 4, "steps": 210,
                                  "kernels": rows}
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({"wrote": args.out, "kernels": len(rows)}))
        return

    def league_step_us(K, opponents, steps, hidden=(128, 64)):
        hp = DQNHParams(batch=BATCH, num_steps=steps)
        r = train_league(ep, [hp] * K, STEP_ENVS, steps, hidden=hidden, opponents=opponents, memory_size=RING,
                         seeds=list(range(K)))
        return K / r.agent_steps_per_s * 1e6

    def single_step_us(steps, hidden=(128, 64)):
        r = train(ep, STEP_ENVS, steps, hidden=hidden, hp=DQNHParams(batch=BATCH, num_steps=steps), memory_size=RING)
        return STEP_ENVS / r.env_steps_per_s * 1e6

    if args.trace_workload:
        league_step_us(2, baselines, 210)
        print(json.dumps({"learners": 2, "opponents": 4, "steps": 210}))
        return
    argv = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and not a.startswith("--out=")
            and (i == 0 or sys.argv[i] != "--out")]
    result = {"command": " ".join(["python", "tools/time_league.py", *argv]), "iters": args.iters, "reps": args.reps,
              "device": torch.cuda.get_device_name(0), "env": "side 11, 6 drones, radius 3 (7x7 windows)",
              "act": {}, "step": {}}

    # ---- 1. the act against drl_pop_act --------------------------------------------------------------------
    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    for E in ENVS_ACT:
        env = BatchedDeliveryDrones(ep, E)
        env.reset(seed=1)
        for t in range(3):
            env.step(env.synth_actions(9, t))
        codes = obs_code_all(env)
        K, N = K_ACT, ep.n_drones
        for name, hidden in NETS.items():
            hps = [DQNHParams(batch=BATCH, epsilon_start=0.1)] * K
            lg = LeagueDQN(294, hidden, hps, E, seeds=list(range(K)))
            pop = PopulationDQN(294, hidden, hps, E, seeds=list(range(K)))
            acts_l = torch.zeros((E, N), dtype=torch.int32, device="cuda")
            acts_p = torch.zeros((K * E, 1), dtype=torch.int32, device="cuda")
            q_l = torch.empty((K, E, 5), device="cuda")
            q_p = torch.empty((K * E, 5), device="cuda")
            rows = codes[:K].reshape(K * E, -1)
            lg.act(codes, 0, seed=3, actions=acts_l, q=q_l)
            pop.act(rows, 0, seed=3, actions=acts_p, q_out=q_p, n_drones=1)
            torch.cuda.synchronize()
            same_q = bool(torch.equal(q_l.view(torch.int32).reshape(-1), q_p.view(torch.int32).reshape(-1)))
            variants = {"league_act": lambda i: lg.act(codes, i, seed=3, actions=acts_l),
                        "pop_act": lambda i: pop.act(rows, i, seed=3, actions=acts_p, n_drones=1)}
            for fn in variants.values():
                timed(fn, 10)
            times = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, args.iters))
            r = {k: summary(v) for k, v in times.items()}
            floor_us = K * E * macs(hidden) * 2 / (PEAK_F32_VECTOR / 2) * 1e6
            for s in r.values():
                s["arithmetic_floor_us"] = floor_us
                s["fraction_of_floor_reached"] = floor_us / s["median_us"]
            r["q_bit_identical"] = same_q
            r["pop_over_league"] = r["pop_act"]["median_us"] / r["league_act"]["median_us"]
            r["league_faster_beyond_both_spreads"] = bool(r["league_act"]["max_us"] < r["pop_act"]["min_us"])
            result["act"][f"{name}_K{K}_E{E}"] = r
            print(f"act {name} K={K} E={E}: league {r['league_act']['median_us']:.1f} us "
                  f"({r['league_act']['min_us']:.1f}..{r['league_act']['max_us']:.1f}), pop {r['pop_act']['median_us']:.1f} us "
                  f"({r['pop_act']['min_us']:.1f}..{r['pop_act']['max_us']:.1f}), x{r['pop_over_league']:.2f}, floor "
                  f"{floor_us:.1f} us, Q identical: {same_q}", flush=True)
            del lg, pop
        del env, codes

    # ---- 2. the league step --------------------------------------------------------------------------------
    variants = {"train_single_agent": lambda n: single_step_us(n),
                "league_K2_4_baselines": lambda n: league_step_us(2, baselines, n),
                "league_K6": lambda n: league_step_us(6, None, n)}
    for fn in variants.values():
        fn(20)
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            times[k].append(fn(args.iters))
    result["step"] = {k: summary(v) for k, v in times.items()}
    result["step"]["envs"], result["step"]["batch"], result["step"]["ring_slots"] = STEP_ENVS, BATCH, RING
    print("step: " + "; ".join(f"{k} {result['step'][k]['median_us']:.1f} us ({result['step'][k]['min_us']:.1f}.."
                               f"{result['step'][k]['max_us']:.1f})" for k in variants), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
