#!/usr/bin/env python3
"""Time the large-batch DQN learner (drl_dqn_large_train, HIP events).

1. The learner call alone: the benchmark net (294-128-64-5) and train_jax.py's
   default net (294-16-16-5), policy-code rows, batches 8, 64, 256, 1024 and
   4096 on a filled 8192-slot ring; beside it, in the same process,
   drl_dqn_train (the single-launch learner) at the batches it takes (8, 64)
   and the same step written in torch ops on `cuda` (the rows gathered by
   index, autograd, the Adam formula, the target copy).  Each figure is the
   median of --reps repetitions of --iters calls, the variants alternating
   inside a repetition; the spread is the repetitions' min..max.
2. --trace-workload runs only 210 learner calls (the benchmark net, --batch):
   the workload of a `rocprofv3 --kernel-trace --stats` run of its own, whose
   kernel_stats CSV a later call records with --stats-csv.

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

NETS = {"128_64": (128, 64), "16_16": (16, 16)}
BATCHES = (8, 64, 256, 1024, 4096)
RING = 8192


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
    from dronerl_amd.dqn import ReplayBuffer, decode_policy_code
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), cap)  # 7x7 windows
    env.reset(seed=0)
    rb = ReplayBuffer(cap, 294, torch.device("cuda"), code_radius=3)
    cur, nxt = env.new_code(), env.new_code()
    env.get_code(out=cur)
    acts = env.synth_actions(seed=9, step=0)
    rew, don = env.step(acts, code=nxt)
    rb.add_many(cur, acts, rew, nxt, don)
    f32 = {"obs": decode_policy_code(rb.obs, 3), "next_obs": decode_policy_code(rb.next_obs, 3)}
    torch.cuda.synchronize()
    assert rb.size == cap
    return rb, f32


def learner_of(hidden, batch, cls):
    from dronerl_amd.dqn import DQNHParams, QNetwork
    net = QNetwork(294, hidden, generator=torch.Generator().manual_seed(0), input="code")
    return cls(net, DQNHParams(batch=batch, num_steps=1000))


def torch_step_of(learner, rb, f32, batch):
    """The same learner block in torch ops on cuda, from the learner's initial parameters."""
    ps = [t.detach().clone().requires_grad_() for wb in learner.params("online") for t in wb]
    tg = [t.detach().clone() for wb in learner.params("target") for t in wb]
    m, v = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    st = {"t": 0}
    hp = learner.hp

    def fwd(q, h):
        for i in range(0, len(q), 2):
            h = h @ q[i].t() + q[i + 1]
            if i < len(q) - 2:
                h = torch.relu(h)
        return h

    def step():
        idx = torch.randint(0, rb.size, (batch,), device="cuda")
        qa = fwd(ps, f32["obs"][idx]).gather(1, rb.actions[idx].long()[:, None])[:, 0]
        with torch.no_grad():
            mx = fwd(tg, f32["next_obs"][idx]).max(dim=1).values
            td = rb.rewards[idx] + hp.gamma * mx * (1 - rb.dones[idx].float())
        loss = ((qa - td) ** 2).mean()
        grads = torch.autograd.grad(loss, ps)
        st["t"] += 1
        t = st["t"]
        with torch.no_grad():
            for p, g, mm, vv in zip(ps, grads, m, v):
                mm.mul_(hp.beta1).add_(g, alpha=1 - hp.beta1)
                vv.mul_(hp.beta2).addcmul_(g, g, value=1 - hp.beta2)
                p.sub_(hp.learning_rate * (mm / (1 - hp.beta1 ** t)) / ((vv / (1 - hp.beta2 ** t)).sqrt() + hp.adam_eps))
            if (t - 1) % hp.target_update_interval == 0:
                for a, b in zip(tg, ps):
                    a.copy_(b)

    return step


def main():
    from dronerl_amd.dqn import DQNLearner, LargeBatchDQNLearner
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--batch", type=int, default=4096, help="--trace-workload: the learner's batch")
    ap.add_argument("--stats-csv", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV to record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "large_batch", "learn.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.stats_csv:  # record the per-launch split of a profiler run of its own beside the timings
        with open(args.out) as f:
            result = json.load(f)
        with open(args.stats_csv) as f:
            rows = [r for r in csv.DictReader(f) if "drl_" in (r.get("Name") or "")]
        result.setdefault("kernel_trace", {})[f"128_64_batch{args.batch}"] = {
            "command": f"rocprofv3 --kernel-trace --stats -- python tools/time_large_learn.py --trace-workload "
                       f"--batch {args.batch}", "learner_calls": 210, "kernels": rows}
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({"wrote": args.out, "kernels": len(rows)}))
        return
    rb, f32 = filled_ring()
    if args.trace_workload:
        learner = learner_of(NETS["128_64"], args.batch, LargeBatchDQNLearner)
        for _ in range(210):
            learner.train(rb)
        torch.cuda.synchronize()
        learner.check_errors()
        print(json.dumps({"learner_calls": 210, "batch": args.batch}))
        return
    result = {"command": " ".join(["python", "tools/time_large_learn.py", *sys.argv[1:]]), "iters": args.iters,
              "reps": args.reps, "device": torch.cuda.get_device_name(0), "ring_slots": RING, "learner_call": {}}
    for name, hidden in NETS.items():
        for batch in BATCHES:
            large = learner_of(hidden, batch, LargeBatchDQNLearner)
            variants = {"large": lambda: large.train(rb), "torch": torch_step_of(large, rb, f32, batch)}
            single = None
            if batch <= 64:  # drl_dqn_train, unchanged, beside it
                single = learner_of(hidden, batch, DQNLearner)
                variants["single_launch"] = lambda: single.train(rb)
            for fn in variants.values():
                timed(fn, 20)
            times = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, args.iters))
            r = {k: summary(v) for k, v in times.items()}
            r["rows_per_s"] = batch / r["large"]["median_us"] * 1e6
            large.check_errors()
            if single is not None:
                single.check_errors()
            result["learner_call"][f"{name}_batch{batch}"] = r
            print(f"{name} batch {batch}: " + ", ".join(
                f"{k} {s['median_us']:.1f} us ({s['min_us']:.1f}..{s['max_us']:.1f})" for k, s in r.items()
                if isinstance(s, dict)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
