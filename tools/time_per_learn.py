#!/usr/bin/env python3
"""Time the prioritized learner (drl_dqn_per_train) beside the uniform one
(drl_dqn_large_train, unchanged) in the same process (HIP events).

1. The learner call alone: the benchmark net (294-128-64-5), policy-code
   rows, a filled 100,000-slot ring, batches 256, 1024 and 4096.  Variants,
   alternating inside a repetition: "uniform" (LargeBatchDQNLearner.train),
   "per" (PrioritizedDQNLearner.train: rebuild x2, sample, the chain, the
   priority update) and "per_mark" (the same after a drl_per_mark_new of
   65,536 rows, a C3 step's add).  Each figure is the median of --reps
   repetitions of --iters calls; the spread is the repetitions' min..max.
2. --trace-workload runs only 210 prioritized learner calls (--batch), each
   after a mark: the workload of a `rocprofv3 --kernel-trace --stats` run of
   its own, whose kernel_stats CSV a later call records with --stats-csv.
3. --learning: 300 steps of 4,096 envs at batch 256 with uniform and with
   prioritized replay (alpha 0.6, beta 0.4 annealed over the run), then the
   greedy eval of each (5 episodes of 2,000 steps); writes both figures.

Writes one JSON file with the command line in the record.
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

HIDDEN = (128, 64)
BATCHES = (256, 1024, 4096)
RING = 100_000
ADD = 65_536  # a C3 training step's transitions


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v),
            "reps_us": v}


def filled_ring(cap=RING):
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import ReplayBuffer
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), cap)  # 7x7 windows
    env.reset(seed=0)
    rb = ReplayBuffer(cap, 294, torch.device("cuda"), code_radius=3)
    cur, nxt = env.new_code(), env.new_code()
    env.get_code(out=cur)
    acts = env.synth_actions(seed=9, step=0)
    rew, don = env.step(acts, code=nxt)
    rb.add_many(cur, acts, rew, nxt, don)
    torch.cuda.synchronize()
    assert rb.size == cap
    return rb


def learner_of(batch, cls):
    from dronerl_amd.dqn import DQNHParams, QNetwork
    net = QNetwork(294, HIDDEN, generator=torch.Generator().manual_seed(0), input="code")
    return cls(net, DQNHParams(batch=batch, num_steps=1000))


def per_of(rb, batch):
    from dronerl_amd.dqn import PrioritizedReplay
    return PrioritizedReplay(rb, alpha=0.6, beta0=0.4, beta_steps=1000, batch=batch)


def learning(out):
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams, QNetwork
    from dronerl_amd.train import evaluate, train
    p, res = EnvParams(), {}
    for name, per in (("uniform", None), ("prioritized", dict(alpha=0.6, beta0=0.4, beta_steps=300, eps=1e-6))):
        r = train(p, 4096, 300, hp=DQNHParams(batch=256, num_steps=300), per=per)
        qnet = QNetwork(294, HIDDEN, precision="f32")
        qnet.load(*zip(*r.learner.params("online")))
        agent, rnd, _ = evaluate(p, qnet, num_evals=5, num_eval_steps=2000, device="cuda")
        res[name] = {"agent_mean": agent[0], "agent_std": agent[1], "random_mean": rnd[0], "random_std": rnd[1],
                     "gap": agent[0] - rnd[0], "loss": r.learner.counters()["loss"]}
        if per is not None:
            res[name]["pmax"] = float(r.replay.pmax.item())
        print(name, json.dumps(res[name]))
    result = {"command": "python tools/time_per_learn.py --learning", "device": torch.cuda.get_device_name(0),
              "what": "300 steps of 4096 envs (EnvParams defaults, net 128-64, batch 256), then the greedy eval of "
                      "drone 0 against random drones: 5 episodes of 2000 steps; one run each (every kernel is "
                      "bit-reproducible)", "runs": res}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": out}))


def main():
    from dronerl_amd.dqn import LargeBatchDQNLearner, PrioritizedDQNLearner
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--batch", type=int, default=4096, help="--trace-workload: the learner's batch")
    ap.add_argument("--stats-csv", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV to record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    per_dir = os.path.join(REPO, "profiles", "per")
    os.makedirs(per_dir, exist_ok=True)
    out = args.out or os.path.join(per_dir, "learning.json" if args.learning else "learn.json")
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.learning:
        return learning(out)
    if args.stats_csv:  # record the per-launch split of a profiler run of its own beside the timings
        with open(out) as f:
            result = json.load(f)
        with open(args.stats_csv) as f:
            rows = [r for r in csv.DictReader(f) if "drl_" in (r.get("Name") or "")]
        result.setdefault("kernel_trace", {})[f"128_64_batch{args.batch}"] = {
            "command": f"rocprofv3 --kernel-trace --stats -- python tools/time_per_learn.py --trace-workload "
                       f"--batch {args.batch}", "learner_calls": 210, "kernels": rows}
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({"wrote": out, "kernels": len(rows)}))
        return
    rb = filled_ring()
    if args.trace_workload:
        learner, per = learner_of(args.batch, PrioritizedDQNLearner), per_of(rb, args.batch)
        for i in range(210):
            per._mark((i * ADD) % RING, ADD)
            learner.train(per)
        torch.cuda.synchronize()
        learner.check_errors()
        print(json.dumps({"learner_calls": 210, "batch": args.batch}))
        return
    result = {"command": " ".join(["python", "tools/time_per_learn.py", *sys.argv[1:]]), "iters": args.iters,
              "reps": args.reps, "device": torch.cuda.get_device_name(0), "ring_slots": RING, "net": "294-128-64-5",
              "learner_call": {}}
    for batch in BATCHES:
        uniform = learner_of(batch, LargeBatchDQNLearner)
        pl, per = learner_of(batch, PrioritizedDQNLearner), per_of(rb, batch)
        pm, per_m = learner_of(batch, PrioritizedDQNLearner), per_of(rb, batch)
        cur = {"c": 0}

        def per_mark():
            per_m._mark(cur["c"], ADD)
            cur["c"] = (cur["c"] + ADD) % RING
            pm.train(per_m)

        variants = {"uniform": lambda: uniform.train(rb), "per": lambda: pl.train(per), "per_mark": per_mark}
        for fn in variants.values():
            timed(fn, 20)
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, args.iters))
        r = {k: summary(v) for k, v in times.items()}
        for k in ("per", "per_mark"):
            r[f"{k}_minus_uniform_us"] = r[k]["median_us"] - r["uniform"]["median_us"]
            # beyond both spreads: the ranges of the repetitions do not overlap
            r[f"{k}_beyond_spreads"] = r[k]["min_us"] > r["uniform"]["max_us"] or r[k]["max_us"] < r["uniform"]["min_us"]
        for lr in (uniform, pl, pm):
            lr.check_errors()
        result["learner_call"][f"batch{batch}"] = r
        print(f"batch {batch}: " + ", ".join(
            f"{k} {s['median_us']:.1f} us ({s['min_us']:.1f}..{s['max_us']:.1f})" for k, s in r.items()
            if isinstance(s, dict)))
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": out}))


if __name__ == "__main__":
    main()
