#!/usr/bin/env python3
"""Time shared-policy self-play with conv learners (HIP events): its act against drl_convleague_act, and its
training step.

1. The act against its yardstick.  For train_jax's default conv net (one 3x3 layer of 8 channels) and the sweep's
   conv net (3x3 layers of 16 and 32 channels, dense 128-64) on 7x7 windows, ONE learner on a team of M = 6 drones
   and E = 4,096 and 65,536 envs: drl_convselfplay_act beside drl_convleague_act (unchanged) with six learners that
   hold copies of the same weights, on the same [6][E] code rows, in the same process: the same rows, the same
   arithmetic.  Before timing, both Q outputs and both action matrices are compared bit for bit (asserted).  Each
   figure is the median of --reps repetitions of --iters calls, the two alternating inside a repetition; the
   spread is the repetitions' min..max.  The expectation, set before any measurement: the self-play act is no
   slower than the league act beyond the two spreads (the same arithmetic, one weight set read instead of six, the
   price one gather index per row).
2. The self-play step (act, opponents' acts, env step, every drone's code, add, train) with the default conv net at
   N = 6, side 11, E = 4,096, batch 8: K = 1 learner on M = 6 drones, and K = 2 learners on M = 2 drones each with
   two sample baselines as opponents; beside them train_league(network_type="conv")'s step for K = 6 learners
   (context, not a bar: six nets learn there, one or two here).  With each: the transitions landed in the rings
   per second.
3. --trace-workload runs only one self-play loop (K = 1, M = 6, 210 steps): the workload of a
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


def _c(out_channels, kernel_size=3, stride=1, padding=1):
    return {"out_channels": out_channels, "kernel_size": kernel_size, "stride": stride, "padding": padding}


# name -> (conv layers, dense widths)
NETS = {"conv8": ((_c(8),), ()), "conv16_32_d128_64": ((_c(16), _c(32)), (128, 64))}
TEAM, ENVS_ACT = 6, (4096, 65536)
STEP_ENVS, BATCH, RING = 4096, 8, 65536
MODELS = os.path.join(REPO, "tests", "golden", "sample_models")


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v),
            "reps_us": v}


def main():
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.evaluator import EVALUATOR_ENV_PARAMS, obs_code_all
    from dronerl_amd.league import ConvLeagueDQN, train_league
    from dronerl_amd.selfplay import ConvSelfPlayDQN, train_selfplay
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--stats-csv", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV to record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_selfplay", "selfplay.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    ep = EnvParams.from_torch_config(dict(EVALUATOR_ENV_PARAMS), window_radius=3)  # 6 drones, side 11, 7x7 windows
    baselines = {4: os.path.join(MODELS, "dqn-agent-2.safetensors"), 5: os.path.join(MODELS, "dqn-agent-3.safetensors")}
    if args.stats_csv:
        with open(args.out) as f:
            result = json.load(f)
        with open(args.stats_csv) as f:
            rows = [r for r in csv.DictReader(f) if "drl_" in (r.get("Name") or "")]
        result["kernel_trace"] = {"command": "rocprofv3 --kernel-trace --stats -- python tools/time_conv_selfplay.py "
                                             "--trace-workload", "learners": 1, "drones_per_learner": TEAM,
                                  "steps": 210, "kernels": rows}
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({"wrote": args.out, "kernels": len(rows)}))
        return

    def selfplay_step_us(K, M, opponents, steps):
        hp = DQNHParams(batch=BATCH, num_steps=steps)
        r = train_selfplay(ep, [hp] * K, M, STEP_ENVS, steps, opponents=opponents, memory_size=RING,
                           seeds=list(range(K)), network_type="conv")
        return K / r.agent_steps_per_s * 1e6

    def league_step_us(K, steps):
        hp = DQNHParams(batch=BATCH, num_steps=steps)
        r = train_league(ep, [hp] * K, STEP_ENVS, steps, memory_size=RING, seeds=list(range(K)), network_type="conv")
        return K / r.agent_steps_per_s * 1e6

    if args.trace_workload:
        selfplay_step_us(1, TEAM, None, 210)
        print(json.dumps({"learners": 1, "drones_per_learner": TEAM, "steps": 210}))
        return
    argv = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and not a.startswith("--out=")
            and (i == 0 or sys.argv[i] != "--out")]
    result = {"command": " ".join(["python", "tools/time_conv_selfplay.py", *argv]), "iters": args.iters,
              "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "env": "side 11, 6 drones, radius 3 (7x7 windows)",
              "expectation": "set in advance: the self-play act is no slower than six league learners beyond the "
                             "two spreads", "act": {}, "step": {}}

    # ---- 1. the act against drl_convleague_act -------------------------------------------------------------
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
        M, N = TEAM, ep.n_drones
        for name, (conv, dense) in NETS.items():
            hp = DQNHParams(batch=BATCH, epsilon_start=0.1)
            sp = ConvSelfPlayDQN((7, 7, 6), conv, dense, [hp], E, team=M, seeds=[0])
            sets = {w: ([p[0] for p in sp.params(w, 0)], [p[1] for p in sp.params(w, 0)]) for w in ("online", "target")}
            lg = ConvLeagueDQN((7, 7, 6), conv, dense, [hp] * M, E, online=[sets["online"]] * M,
                               target=[sets["target"]] * M)
            acts_s = torch.zeros((E, N), dtype=torch.int32, device="cuda")
            acts_l = torch.zeros((E, N), dtype=torch.int32, device="cuda")
            q_s = torch.empty((1, M, E, 5), device="cuda")
            q_l = torch.empty((M, E, 5), device="cuda")
            sp.act(codes, 0, seed=3, actions=acts_s, q=q_s)
            lg.act(codes, 0, seed=3, actions=acts_l, q=q_l)
            torch.cuda.synchronize()
            same_q = bool(torch.equal(q_s.view(torch.int32).reshape(-1), q_l.view(torch.int32).reshape(-1)))
            assert same_q and torch.equal(acts_s, acts_l), "the self-play act differs from six league learners"
            variants = {"selfplay_act": lambda i: sp.act(codes, i, seed=3, actions=acts_s),
                        "league_act": lambda i: lg.act(codes, i, seed=3, actions=acts_l)}
            for fn in variants.values():
                timed(fn, 10)
            times = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, args.iters))
            r = {k: summary(v) for k, v in times.items()}
            r["q_bit_identical"] = same_q
            r["env_tile"] = sp.act_plan["env_tile"]
            r["league_over_selfplay"] = r["league_act"]["median_us"] / r["selfplay_act"]["median_us"]
            # "no slower beyond the two spreads": the self-play repetitions do not all lie above the league's
            r["selfplay_slower_beyond_both_spreads"] = bool(r["selfplay_act"]["min_us"] > r["league_act"]["max_us"])
            r["selfplay_faster_beyond_both_spreads"] = bool(r["selfplay_act"]["max_us"] < r["league_act"]["min_us"])
            r["expectation_held"] = not r["selfplay_slower_beyond_both_spreads"]
            result["act"][f"{name}_M{M}_E{E}"] = r
            print(f"act {name} M={M} E={E}: self-play {r['selfplay_act']['median_us']:.1f} us "
                  f"({r['selfplay_act']['min_us']:.1f}..{r['selfplay_act']['max_us']:.1f}), league x6 "
                  f"{r['league_act']['median_us']:.1f} us ({r['league_act']['min_us']:.1f}.."
                  f"{r['league_act']['max_us']:.1f}), x{r['league_over_selfplay']:.3f}, Q identical: {same_q}, "
                  f"expectation held: {r['expectation_held']}", flush=True)
            del sp, lg
        del env, codes

    # ---- 2. the self-play step -----------------------------------------------------------------------------
    variants = {"selfplay_K1_M6": (lambda n: selfplay_step_us(1, 6, None, n), 6),
                "selfplay_K2_M2_2_baselines": (lambda n: selfplay_step_us(2, 2, baselines, n), 4),
                "league_K6": (lambda n: league_step_us(6, n), 6)}
    for fn, _ in variants.values():
        fn(20)
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, (fn, _) in variants.items():
            times[k].append(fn(args.iters))
    result["step"] = {k: summary(v) for k, v in times.items()}
    for k, (_, drones) in variants.items():
        result["step"][k]["ring_rows_per_step"] = drones * STEP_ENVS
        result["step"][k]["ring_rows_per_s"] = drones * STEP_ENVS / (result["step"][k]["median_us"] * 1e-6)
    result["step"]["envs"], result["step"]["batch"], result["step"]["ring_slots"] = STEP_ENVS, BATCH, RING
    result["step"]["net"] = "conv8"
    print("step: " + "; ".join(f"{k} {result['step'][k]['median_us']:.1f} us ({result['step'][k]['min_us']:.1f}.."
                               f"{result['step'][k]['max_us']:.1f}), {result['step'][k]['ring_rows_per_s'] / 1e6:.1f} M rows/s"
                               for k in variants), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
