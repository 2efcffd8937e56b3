#!/usr/bin/env python3
"""Time the prioritized conv learner (drl_convnet_dqn_per_train) beside the
uniform one (drl_convnet_dqn_large_train, unchanged) in the same process
(HIP events), on the pattern of tools/time_per_learn.py.

1. The learner call alone: train_jax's default conv net and the sweep's conv
   net on 7 x 7 policy-code rows, a filled and wholly marked 100,000-slot
   ring, batches 256 and 1024.  Variants, alternating inside a repetition:
   "uniform" (LargeBatchConvDQNLearner.train) and "per"
   (PrioritizedConvDQNLearner.train: rebuild x2, sample, the chain, the
   priority update).  Each figure is the median of --reps repetitions of
   --iters calls; the spread is the repetitions' min..max.
   --wide: the same comparison for drl_widenet_dqn_per_train beside
   drl_widenet_dqn_train on the sweep's dense net (294-256-128-64-5),
   recorded under "wide_learner_call" of the same file.
   The expectation, stated before measuring: priorities add what they add to
   the dense learner, +20..45 us per call, beyond both spreads; each entry
   records whether it was met.
2. --learning: tools/train_eval.py's settings behind
   profiles/conv_large/learning.json (EnvParams(n_drones=4, grid_size=9),
   4,096 envs, 300 steps, batch 256, the default conv net) once with uniform
   and once with prioritized replay (alpha 0.6, beta 0.4 annealed over the
   run), then the greedy eval of each (5 episodes of 2,000 steps).

Writes profiles/conv_per/learn.json (or learning.json) with the command line
in the record.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

_K3 = dict(kernel_size=3, stride=1, padding=1)
NETS = {"train_jax_default": (({"out_channels": 8, **_K3},), ()),
        "sweep": (({"out_channels": 16, **_K3}, {"out_channels": 32, **_K3}), (128, 64))}
WIDE_HIDDEN = (256, 128, 64)
BATCHES = (256, 1024)
RING = 100_000
EXPECT_US = (20.0, 45.0)


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


def conv_learner(cls, net_id, batch):
    from dronerl_amd.dqn import ConvQNetwork, DQNHParams
    conv, dense = NETS[net_id]
    net = ConvQNetwork((7, 7, 6), conv, dense, generator=torch.Generator().manual_seed(0), input="code")
    return cls(net, DQNHParams(batch=batch, num_steps=1000))


def wide_learner(cls, batch):
    from dronerl_amd.dqn import DQNHParams, WideQNetwork
    net = WideQNetwork(294, WIDE_HIDDEN, generator=torch.Generator().manual_seed(0), input="code")
    return cls(net, DQNHParams(batch=batch, num_steps=1000))


def compare(uniform, pl, rb, batch, iters, reps):
    """The two learners' calls, alternating inside a repetition."""
    from dronerl_amd.dqn import PrioritizedReplay
    per = PrioritizedReplay(rb, alpha=0.6, beta0=0.4, beta_steps=1000, batch=batch)
    variants = {"uniform": lambda: uniform.train(rb), "per": lambda: pl.train(per)}
    for fn in variants.values():
        timed(fn, 20)
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    r = {k: summary(v) for k, v in times.items()}
    added = r["per"]["median_us"] - r["uniform"]["median_us"]
    r["per_minus_uniform_us"] = added
    # beyond both spreads: the ranges of the repetitions do not overlap
    r["per_beyond_spreads"] = r["per"]["min_us"] > r["uniform"]["max_us"] or r["per"]["max_us"] < r["uniform"]["min_us"]
    r["expected_us"] = list(EXPECT_US)
    r["expectation_met"] = bool(r["per_beyond_spreads"] and EXPECT_US[0] <= added <= EXPECT_US[1])
    for lr in (uniform, pl):
        lr.check_errors()
    print(", ".join(f"{k} {s['median_us']:.1f} us ({s['min_us']:.1f}..{s['max_us']:.1f})" for k, s in r.items()
                    if isinstance(s, dict)) + f", added {added:.1f} us, expectation "
          + ("met" if r["expectation_met"] else "missed"))
    return r


def learning(out):
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import ConvQNetwork, DQNHParams
    from dronerl_amd.train import evaluate, train
    p, res = EnvParams(n_drones=4, grid_size=9), {}
    for name, per in (("uniform", None), ("prioritized", dict(alpha=0.6, beta0=0.4, beta_steps=300, eps=1e-6))):
        r = train(p, 4096, 300, network_type="conv", hp=DQNHParams(batch=256, num_steps=300), per=per)
        qnet = ConvQNetwork(r.net.obs_shape, r.net.conv_layers, r.net.dense_layers)
        qnet.load(r.net.conv_weights, r.net.conv_biases, r.net.weights, r.net.biases)
        agent, rnd, _ = evaluate(p, qnet, num_evals=5, num_eval_steps=2000, device="cuda")
        res[name] = {"learner": type(r.learner).__name__, "agent_mean": agent[0], "agent_std": agent[1],
                     "random_mean": rnd[0], "random_std": rnd[1], "gap": agent[0] - rnd[0],
                     "loss": r.learner.counters()["loss"], "env_steps_per_s": r.env_steps_per_s}
        if per is not None:
            res[name]["pmax"] = float(r.replay.pmax.item())
        print(name, json.dumps(res[name]))
    result = {"command": "python tools/time_conv_per_learn.py --learning", "device": torch.cuda.get_device_name(0),
              "what": "EnvParams(n_drones=4, grid_size=9), 4096 envs, 300 steps, network_type conv (the default net), "
                      "batch 256, then the greedy eval of drone 0 against random drones: 5 episodes of 2000 steps; "
                      "one run each (every kernel is bit-reproducible)",
              "prioritized_minus_uniform_gap": res["prioritized"]["gap"] - res["uniform"]["gap"], "runs": res}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": out}))


def main():
    from dronerl_amd.dqn import (LargeBatchConvDQNLearner, PrioritizedConvDQNLearner, PrioritizedWideDQNLearner,
                                 WideDQNLearner)
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--wide", action="store_true", help="the wide dense learner's comparison (added to --out)")
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_dir = os.path.join(REPO, "profiles", "conv_per")
    os.makedirs(out_dir, exist_ok=True)
    out = args.out or os.path.join(out_dir, "learning.json" if args.learning else "learn.json")
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.learning:
        return learning(out)
    rb = filled_ring()
    command = " ".join(["python", "tools/time_conv_per_learn.py", *sys.argv[1:]])
    if args.wide:
        try:
            with open(out) as f:
                result = json.load(f)
        except OSError:
            result = {}
        section = {"command": command, "iters": args.iters, "reps": args.reps,
                   "device": torch.cuda.get_device_name(0), "ring_slots": RING, "net": "294-256-128-64-5"}
        for batch in BATCHES:
            print(f"wide batch {batch}: ", end="")
            section[f"batch{batch}"] = compare(wide_learner(WideDQNLearner, batch),
                                               wide_learner(PrioritizedWideDQNLearner, batch), rb, batch, args.iters,
                                               args.reps)
        result["wide_learner_call"] = section
    else:
        result = {"command": command, "iters": args.iters, "reps": args.reps,
                  "device": torch.cuda.get_device_name(0), "ring_slots": RING,
                  "expectation": "stated before measuring: the priorities add +20..45 us per call (rebuild x2, "
                                 "sample, priority), beyond both spreads", "learner_call": {}}
        for net_id in NETS:
            for batch in BATCHES:
                print(f"{net_id} batch {batch}: ", end="")
                result["learner_call"][f"{net_id}_batch{batch}"] = compare(
                    conv_learner(LargeBatchConvDQNLearner, net_id, batch),
                    conv_learner(PrioritizedConvDQNLearner, net_id, batch), rb, batch, args.iters, args.reps)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": out}))


if __name__ == "__main__":
    main()
