#!/usr/bin/env python3
"""Time the conv DQN learner at replay batches up to 4096
(drl_convnet_dqn_large_train, HIP events).

1. The learner call alone on a filled 4,096-slot policy-code ring (1,024 envs
   x 4 steps), for train_jax.py's default conv net (conv 6->8 k3 p1, the
   flatten into the Q head), the reference's dqn-agent-5 shape (conv 6->4 k3
   p1, dense 8) and run_jax_sweep.py's conv net (conv 6->16->32 k3 p1, dense
   128-64), at batches 8, 64, 256, 1024 and 4096; in the same process
   drl_convnet_dqn_train at batches 8 and 64 (the learner make_learner keeps
   up to 64) and the same step written in torch ops on `cuda` (the rows
   gathered by index, autograd, the Adam formula, the target copy).  Each
   figure is the median of --reps repetitions of --iters calls, the variants
   alternating inside a repetition; the spread is the repetitions' min..max.
   The bar: from batch 256 up the new call is faster than the torch step by
   more than both spreads.
2. --learning: train(EnvParams(n_drones=4, grid_size=9), 4096 envs, 300 steps,
   network_type="conv") at batch 256 and at batch 8 in one process, each
   followed by evaluate(5 episodes x 2000 steps): the greedy agent's gap over
   the random drones.
3. --trace-workload NET BATCH runs only 50 learner calls: the workload of a
   `rocprofv3 --kernel-trace --stats` run of its own, whose kernel_stats CSV
   a later call records with --stats-csv (and --trace-workload for its name).

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

_K3 = dict(kernel_size=3, stride=1, padding=1)
NETS = {"train_jax_default": (({"out_channels": 8, **_K3},), ()),
        "agent5": (({"out_channels": 4, **_K3},), (8,)),
        "sweep": (({"out_channels": 16, **_K3}, {"out_channels": 32, **_K3}), (128, 64))}
BATCHES = (8, 64, 256, 1024, 4096)
TRACE_CALLS = 50


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


def filled_ring(cap=4096, envs=1024, steps=4):
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import ReplayBuffer, decode_policy_code
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), envs)  # 7x7 windows
    env.reset(seed=0)
    rb = ReplayBuffer(cap, 294, torch.device("cuda"), code_radius=3)
    cur, nxt = env.new_code(), env.new_code()
    env.get_code(out=cur)
    for t in range(steps):
        acts = env.synth_actions(seed=9, step=t)
        rew, don = env.step(acts, code=nxt)
        rb.add_many(cur, acts, rew, nxt, don)
        cur, nxt = nxt, cur
    f32 = {"obs": decode_policy_code(rb.obs, 3), "next_obs": decode_policy_code(rb.next_obs, 3)}
    torch.cuda.synchronize()
    assert rb.size == cap
    return rb, f32


def learner_of(cls, conv, dense, batch):
    from dronerl_amd.dqn import ConvQNetwork, DQNHParams
    net = ConvQNetwork((7, 7, 6), conv, dense, generator=torch.Generator().manual_seed(0), input="code")
    return cls(net, DQNHParams(batch=batch, num_steps=1000))


def torch_step_of(conv, learner, rb, f32, batch):
    """The same learner block in torch ops on cuda, from the learner's initial parameters."""
    F = torch.nn.functional
    ps = [t.detach().clone().requires_grad_() for wb in learner.params("online") for t in wb]
    tg = [t.detach().clone() for wb in learner.params("target") for t in wb]
    m, v = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    st = {"t": 0}
    hp = learner.hp

    def fwd(q, x):
        h = x.reshape(-1, 7, 7, 6).permute(0, 3, 1, 2)
        for i, c in enumerate(conv):
            h = torch.relu(F.conv2d(h, q[2 * i], q[2 * i + 1], stride=c["stride"], padding=c["padding"]))
        h = h.flatten(1)
        rest = q[2 * len(conv):]
        for i in range(0, len(rest), 2):
            h = h @ rest[i].t() + rest[i + 1]
            if i < len(rest) - 2:
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


def learning():
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import ConvQNetwork, DQNHParams
    from dronerl_amd.train import evaluate, train
    p = EnvParams(n_drones=4, grid_size=9)
    out = {}
    for batch in (256, 8):
        res = train(p, 4096, 300, network_type="conv", hp=DQNHParams(batch=batch, num_steps=300))
        qnet = ConvQNetwork(res.net.obs_shape, res.net.conv_layers, res.net.dense_layers)
        qnet.load(res.net.conv_weights, res.net.conv_biases, res.net.weights, res.net.biases)
        agent, rnd, _ = evaluate(p, qnet, num_evals=5, num_eval_steps=2000, device="cuda")
        out[f"batch{batch}"] = {"learner": type(res.learner).__name__, "agent_mean": agent[0], "agent_std": agent[1],
                                "random_mean": rnd[0], "random_std": rnd[1], "gap": agent[0] - rnd[0]}
        print(f"batch {batch} ({type(res.learner).__name__}): agent {agent[0]:.4f} +- {agent[1]:.4f}, random "
              f"{rnd[0]:.4f} +- {rnd[1]:.4f}, gap {agent[0] - rnd[0]:.4f}")
    return out


def write(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": path}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--trace-workload", nargs=2, metavar=("NET", "BATCH"), default=None)
    ap.add_argument("--stats-csv", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV to record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    from dronerl_amd.dqn import ConvDQNLearner, LargeBatchConvDQNLearner
    command = " ".join(["python", "tools/time_conv_large_learn.py", *sys.argv[1:]])
    prof = os.path.join(REPO, "profiles", "conv_large")
    if args.stats_csv:  # record the per-launch split of a profiler run of its own
        net, batch = args.trace_workload
        with open(args.stats_csv) as f:
            rows = [r for r in csv.DictReader(f) if "drl_" in (r.get("Name") or "")]
        write(args.out or os.path.join(prof, f"kernel_trace_{net}_batch{batch}.json"),
              {"command": "rocprofv3 --kernel-trace --stats -- python tools/time_conv_large_learn.py "
                          f"--trace-workload {net} {batch}", "learner_calls": TRACE_CALLS, "kernels": rows})
        return
    if args.learning:
        write(args.out or os.path.join(prof, "learning.json"),
              {"command": command, "device": torch.cuda.get_device_name(0), "train": "EnvParams(n_drones=4, "
               "grid_size=9), 4096 envs, 300 steps, network_type conv; evaluate 5 x 2000", "runs": learning()})
        return
    rb, f32 = filled_ring()
    if args.trace_workload:
        net, batch = args.trace_workload
        learner = learner_of(LargeBatchConvDQNLearner, *NETS[net], int(batch))
        for _ in range(TRACE_CALLS):
            learner.train(rb)
        torch.cuda.synchronize()
        learner.check_errors()
        print(json.dumps({"learner_calls": TRACE_CALLS}))
        return
    result = {"command": command, "iters": args.iters, "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "learner_call": {}}
    for name, (conv, dense) in NETS.items():
        for batch in BATCHES:
            learner = learner_of(LargeBatchConvDQNLearner, conv, dense, batch)
            variants = {"device": lambda: learner.train(rb),
                        "torch": torch_step_of(conv, learner, rb, f32, batch)}
            if batch <= 64:
                old = learner_of(ConvDQNLearner, conv, dense, batch)
                variants["conv_learner"] = lambda: old.train(rb)
            for fn in variants.values():
                timed(fn, 20)
            times = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, fn in variants.items():
                    times[k].append(timed(fn, args.iters))
            r = {k: summary(v) for k, v in times.items()}
            r["faster_than_torch_by_us"] = r["torch"]["median_us"] - r["device"]["median_us"]
            r["faster_than_torch_beyond_spread"] = bool(
                r["faster_than_torch_by_us"] > max(r["torch"]["spread_us"], r["device"]["spread_us"]))
            learner.check_errors()
            result["learner_call"][f"{name}_batch{batch}"] = r
            line = (f"{name} batch {batch}: large learner call {r['device']['median_us']:.1f} us "
                    f"({r['device']['min_us']:.1f}..{r['device']['max_us']:.1f}), torch step "
                    f"{r['torch']['median_us']:.1f} us ({r['torch']['min_us']:.1f}..{r['torch']['max_us']:.1f})")
            if "conv_learner" in r:
                c = r["conv_learner"]
                line += f", drl_convnet_dqn_train {c['median_us']:.1f} us ({c['min_us']:.1f}..{c['max_us']:.1f})"
            print(line, flush=True)
    write(args.out or os.path.join(prof, "learn.json"), result)


if __name__ == "__main__":
    main()
