#!/usr/bin/env python3
"""Time the Double DQN learner calls beside the max-rule calls of the same family in the same process (HIP
events), and report what the rule does to learning on this game.

1. The learner call alone (default): policy-code rows, a filled 100,000-slot ring, batches 8, 256, 1024 and 4096.
   Families: "dense" (net 128-64: drl_dqn_double_train beside drl_dqn_large_train), "wide" (net 256-128-64:
   drl_widenet_dqn_double_train beside drl_widenet_dqn_train) and "per" (net 128-64 on prioritized rows:
   drl_dqn_double_per_train beside drl_dqn_per_train).  The two rules alternate inside a repetition; each figure
   is the median of --reps repetitions of --iters calls, the spread is the repetitions' min..max, and a
   difference counts as real only beyond both spreads (the ranges do not overlap).
2. --trace-workload runs only 210 Double learner calls (--batch, the dense family): the workload of a
   `rocprofv3 --kernel-trace --stats` run of its own.
3. --population: time_population.py's figures at P = 64 (8 envs per member, batch 8, net 128-64) with half the
   members Double beside the all-max population, alternating.
4. --learning: 300 steps of 4,096 envs at batch 256 with train_jax's defaults, Double against the max rule,
   uniform and prioritized replay, one seed each, through tools/train_eval.py's path (train, save in the
   reference's torch format, reload, greedy eval of 5 episodes of 2,000 steps).

Writes one JSON file with the command line in the record.  bench.py does not time this path.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

BATCHES = (8, 256, 1024, 4096)
RING = 100_000
FAMILIES = {"dense": (128, 64), "wide": (256, 128, 64), "per": (128, 64)}


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


def learner_of(family, batch, double):
    from dronerl_amd import dqn
    hp = dqn.DQNHParams(batch=batch, num_steps=1000, double_dqn=double)
    g = torch.Generator().manual_seed(0)
    if family == "wide":
        return dqn.WideDQNLearner(dqn.WideQNetwork(294, FAMILIES[family], generator=g, input="code"), hp)
    cls = dqn.PrioritizedDQNLearner if family == "per" else dqn.LargeBatchDQNLearner
    return cls(dqn.QNetwork(294, FAMILIES[family], generator=g, input="code"), hp)


def write(out, result):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": out}))


def command():
    argv = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]
    return " ".join(["python", "tools/time_double_learn.py", *argv])


def beyond(a, b):
    """The two figures' repetitions do not overlap."""
    return bool(a["min_us"] > b["max_us"] or a["max_us"] < b["min_us"])


def learner_calls(args, out):
    from dronerl_amd.dqn import PrioritizedReplay
    rb = filled_ring()
    result = {"command": command(), "iters": args.iters, "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "ring_slots": RING, "rows": "policy code, 7x7 window", "families": {}}
    for family, hidden in FAMILIES.items():
        fam = {}
        for batch in BATCHES:
            mx, dbl = learner_of(family, batch, False), learner_of(family, batch, True)
            if family == "per":
                pm = PrioritizedReplay(rb, alpha=0.6, beta0=0.4, beta_steps=1000, batch=batch)
                pd = PrioritizedReplay(rb, alpha=0.6, beta0=0.4, beta_steps=1000, batch=batch)
                variants = {"max": lambda: mx.train(pm), "double": lambda: dbl.train(pd)}
            else:
                variants = {"max": lambda: mx.train(rb), "double": lambda: dbl.train(rb)}
            for fn in variants.values():
                timed(fn, 20)
            times = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, args.iters))
            r = {k: summary(v) for k, v in times.items()}
            r["double_minus_max_us"] = r["double"]["median_us"] - r["max"]["median_us"]
            r["beyond_both_spreads"] = beyond(r["double"], r["max"])
            mx.check_errors()
            dbl.check_errors()
            fam[f"batch{batch}"] = r
            print(f"{family} {'-'.join(map(str, hidden))} batch {batch}: max {r['max']['median_us']:.1f} us "
                  f"({r['max']['min_us']:.1f}..{r['max']['max_us']:.1f}), double {r['double']['median_us']:.1f} us "
                  f"({r['double']['min_us']:.1f}..{r['double']['max_us']:.1f}), {r['double_minus_max_us']:+.1f} us, "
                  f"beyond both spreads: {r['beyond_both_spreads']}", flush=True)
        result["families"][family] = {"net": "294-" + "-".join(map(str, hidden)) + "-5", **fam}
    write(out, result)


def population(args, out):
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.population import train_population
    ep, P, E, B = EnvParams(n_drones=4, grid_size=9, window_radius=3), 64, 8, 8

    def step_us(half_double, steps):
        hps = [DQNHParams(batch=B, num_steps=steps, double_dqn=bool(half_double and m % 2)) for m in range(P)]
        r = train_population(ep, hps, E, steps, hidden=(128, 64), memory_size=4096, seeds=list(range(P)))
        return P / r.agent_steps_per_s * 1e6

    variants = {"all_max": lambda: step_us(False, args.iters), "half_double": lambda: step_us(True, args.iters)}
    step_us(False, 20)
    step_us(True, 20)
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            times[k].append(fn())
    r = {k: summary(v) for k, v in times.items()}
    r["half_double_minus_all_max_us"] = r["half_double"]["median_us"] - r["all_max"]["median_us"]
    r["beyond_both_spreads"] = beyond(r["half_double"], r["all_max"])
    print(json.dumps({k: (v if not isinstance(v, dict) else {x: v[x] for x in ("median_us", "min_us", "max_us")})
                      for k, v in r.items()}))
    write(out, {"command": command(), "iters": args.iters, "reps": args.reps, "device": torch.cuda.get_device_name(0),
                "members": P, "envs_per_member": E, "batch": B, "net": "294-128-64-5", "env": "9x9, 4 drones, radius 3",
                "what": "one population training step (act, env step, add, train); half_double: odd members Double",
                "step": r})


def learning(out):
    from dronerl_amd import EnvParams
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.train import evaluate, train
    p, res = EnvParams(), {}
    for per_name, per in (("uniform", None), ("prioritized", dict(alpha=0.6, beta0=0.4, beta_steps=300, eps=1e-6))):
        for rule, double in (("max", False), ("double", True)):
            r = train(p, 4096, 300, hp=DQNHParams(batch=256, num_steps=300), per=per, double_dqn=double)
            with tempfile.TemporaryDirectory() as d:  # (tools/train_eval.py's path: save, reload, evaluate)
                path = os.path.join(d, "agent.safetensors")
                r.learner.save(path, format="torch")
                qnet = to_qnet(read_checkpoint(path), device="cuda")
            agent, rnd, _ = evaluate(p, qnet, num_evals=5, num_eval_steps=2000, device="cuda")
            name = f"{per_name}_{rule}"
            res[name] = {"agent_mean": agent[0], "agent_std": agent[1], "random_mean": rnd[0], "random_std": rnd[1],
                         "gap": agent[0] - rnd[0], "loss": r.learner.counters()["loss"],
                         "learner": type(r.learner).__name__, "double_dqn": bool(r.learner.hp.double_dqn)}
            print(name, json.dumps(res[name]), flush=True)
    write(out, {"command": command(), "device": torch.cuda.get_device_name(0),
                "what": "300 steps of 4096 envs (EnvParams defaults, net 128-64, batch 256, train_jax's other "
                        "defaults), then the greedy eval of drone 0 against random drones through a saved and "
                        "reloaded checkpoint: 5 episodes of 2000 steps; one seed each, nothing tuned", "runs": res})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--population", action="store_true")
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--batch", type=int, default=4096, help="--trace-workload: the learner's batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    name = "learning.json" if args.learning else "population.json" if args.population else "learn.json"
    out = args.out or os.path.join(REPO, "profiles", "double_dqn", name)
    if args.learning:
        return learning(out)
    if args.population:
        return population(args, out)
    if args.trace_workload:
        rb = filled_ring()
        learner = learner_of("dense", args.batch, True)
        for _ in range(210):
            learner.train(rb)
        torch.cuda.synchronize()
        learner.check_errors()
        print(json.dumps({"learner_calls": 210, "batch": args.batch}))
        return
    learner_calls(args, out)


if __name__ == "__main__":
    main()
