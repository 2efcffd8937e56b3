#!/usr/bin/env python3
"""Time the conv league (HIP events): its act against drl_convpop_act, and its training step.

1. The act against its yardstick.  For train_jax's default conv net and the sweep's conv net
   (tools/time_conv_population.py NETS) on 7x7 windows, K = 6 learners and E = 4,096 and 65,536 envs:
   drl_convleague_act beside drl_convpop_act (unchanged; members = K, envs_per_member = E) on the same K * E code
   rows, the same parameters, in the same process.  Before timing, both Q outputs are compared bit for bit (an
   assertion).  Each figure is the median of --reps repetitions of --iters calls, the two alternating inside a
   repetition; the spread is the repetitions' min..max.  The new act counts as faster where its max is below the
   other's min.  Beside each time: the arithmetic floor (the learner's order needs a separate multiply and add
   per product: 2 FLOP per MAC at half the 157.3 TF f32 vector peak) and the fraction of it reached.
2. The league step (act, opponents' acts, env step, every drone's code, add, train) at N = 6, side 11,
   E = 4,096, batch 8, for each net: K = 2 learners with 4 sample baselines as opponents, and K = 6 learners.
3. --trace-workload runs only one league loop (train_jax's default net, K = 2 with 4 opponents, 210 steps): the
   workload of a `rocprofv3 --kernel-trace --stats` run of its own, whose kernel_stats CSV a later call records
   with --stats-csv (the per-launch split of one step).

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

from tools.time_conv_population import NETS  # noqa: E402

K_ACT, ENVS_ACT = 6, (4096, 65536)
STEP_ENVS, BATCH, RING = 4096, 8, 65536
TRACE_NET = "train_jax_default_8"
MODELS = os.path.join(REPO, "tests", "golden", "sample_models")
PEAK_F32_VECTOR = 157.3e12  # MI355X vector f32 peak (packed FMA): a multiply and an add per product run at half


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v),
            "reps_us": v}


def macs(conv, dense, W=7, A=5):
    """Products of one forward, padding taps included (an upper bound of the taps inside the map)."""
    total, side, cin = 0, W, 6
    for c in conv:
        k, co = c["kernel_size"], c["out_channels"]
        side = (side + 2 * c["padding"] - k) // c["stride"] + 1
        total += side * side * co * cin * k * k
        cin = co
    sizes = [side * side * cin, *dense, A]
    return total + sum(sizes[i] * sizes[i + 1] for i in range(len(sizes) - 1))


def main():
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.evaluator import EVALUATOR_ENV_PARAMS, obs_code_all
    from dronerl_amd.league import ConvLeagueDQN, train_league
    from dronerl_amd.population import ConvPopulationDQN
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--stats-csv", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV to record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_league", "league.json"))
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
        result["kernel_trace"] = {"command": "rocprofv3 --kernel-trace --stats -- python tools/time_conv_league.py "
                                             "--trace-workload", "net": TRACE_NET, "learners": 2, "opponents": 4,
                                  "steps": 210, "kernels": rows}
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({"wrote": args.out, "kernels": len(rows)}))
        return

    def league_step_us(net, K, opponents, steps):
        conv, dense = net
        hp = DQNHParams(batch=BATCH, num_steps=steps)
        r = train_league(ep, [hp] * K, STEP_ENVS, steps, opponents=opponents, memory_size=RING, seeds=list(range(K)),
                         network_type="conv", conv_layers=conv, conv_dense_layers=dense)
        return K / r.agent_steps_per_s * 1e6

    if args.trace_workload:
        league_step_us(NETS[TRACE_NET], 2, baselines, 210)
        print(json.dumps({"net": TRACE_NET, "learners": 2, "opponents": 4, "steps": 210}))
        return
    argv = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and not a.startswith("--out=")
            and (i == 0 or sys.argv[i] != "--out")]
    result = {"command": " ".join(["python", "tools/time_conv_league.py", *argv]), "iters": args.iters,
              "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "env": "side 11, 6 drones, radius 3 (7x7 windows)", "act": {}, "step": {}}

    # ---- 1. the act against drl_convpop_act ----------------------------------------------------------------
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
        for name, (conv, dense) in NETS.items():
            hps = [DQNHParams(batch=BATCH, epsilon_start=0.1)] * K
            lg = ConvLeagueDQN((7, 7, 6), conv, dense, hps, E, seeds=list(range(K)))
            plan = lg.act_plan
            acts_l = torch.zeros((E, N), dtype=torch.int32, device="cuda")
            acts_p = torch.zeros((K * E, 1), dtype=torch.int32, device="cuda")
            q_l = torch.empty((K, E, 5), device="cuda")
            q_p = torch.empty((K * E, 5), device="cuda")
            rows = codes[:K].reshape(K * E, -1)

            def pop_act(i, q_out=None):  # drl_convpop_act on the same block: K members, E envs each
                ConvPopulationDQN.act(lg, rows, i, seed=3, actions=acts_p, q_out=q_out, n_drones=1)

            lg.act(codes, 0, seed=3, actions=acts_l, q=q_l)
            pop_act(0, q_p)
            torch.cuda.synchronize()
            same_q = bool(torch.equal(q_l.view(torch.int32).reshape(-1), q_p.view(torch.int32).reshape(-1)))
            assert same_q, f"{name} E={E}: drl_convleague_act's Q differs from drl_convpop_act's"
            variants = {"convleague_act": lambda i: lg.act(codes, i, seed=3, actions=acts_l), "convpop_act": pop_act}
            for fn in variants.values():
                timed(fn, 5)
            times = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, args.iters))
            r = {k: summary(v) for k, v in times.items()}
            floor_us = K * E * macs(conv, dense) * 2 / (PEAK_F32_VECTOR / 2) * 1e6
            for s in r.values():
                s["arithmetic_floor_us"] = floor_us
                s["fraction_of_floor_reached"] = floor_us / s["median_us"]
            r["q_bit_identical"] = same_q
            r["plan"] = plan
            r["convpop_over_convleague"] = r["convpop_act"]["median_us"] / r["convleague_act"]["median_us"]
            r["convleague_faster_beyond_both_spreads"] = bool(r["convleague_act"]["max_us"] < r["convpop_act"]["min_us"])
            result["act"][f"{name}_K{K}_E{E}"] = r
            a, b = r["convleague_act"], r["convpop_act"]
            print(f"act {name} K={K} E={E} (T={plan['env_tile']}, {plan['threads']} threads): convleague "
                  f"{a['median_us']:.1f} us ({a['min_us']:.1f}..{a['max_us']:.1f}), convpop {b['median_us']:.1f} us "
                  f"({b['min_us']:.1f}..{b['max_us']:.1f}), x{r['convpop_over_convleague']:.2f}, floor {floor_us:.1f} us, "
                  f"Q identical: {same_q}", flush=True)
            del lg
        del env, codes

    # ---- 2. the league step --------------------------------------------------------------------------------
    for name, net in NETS.items():
        variants = {"league_K2_4_baselines": lambda n: league_step_us(net, 2, baselines, n),
                    "league_K6": lambda n: league_step_us(net, 6, None, n)}
        for fn in variants.values():
            fn(20)
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                times[k].append(fn(args.iters))
        result["step"][name] = {k: summary(v) for k, v in times.items()}
        print(f"step {name}: " + "; ".join(f"{k} {s['median_us']:.1f} us ({s['min_us']:.1f}..{s['max_us']:.1f})"
                                           for k, s in result["step"][name].items()), flush=True)
    result["step"]["envs"], result["step"]["batch"], result["step"]["ring_slots"] = STEP_ENVS, BATCH, RING
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
