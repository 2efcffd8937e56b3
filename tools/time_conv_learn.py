#!/usr/bin/env python3
"""Time the conv DQN learner (drl_convnet_dqn_train, HIP events) and the
train loop around it.

1. The learner call alone: the reference's dqn-agent-5 shape (conv 6->4 k3 p1,
   dense 8) and train_jax.py's default conv net (conv 6->8 k3 p1, the flatten
   into the Q head), policy-code rows, batches 8 and 64, on a filled 300-slot
   ring, beside the same step written in torch ops on `cuda` (the rows
   gathered by index, autograd, the Adam formula, the target copy) in the same
   process -- the only other way to train these nets on the GPU.  Each figure
   is the median of --reps repetitions of --iters calls, the variants
   alternating inside a repetition; the spread is the repetitions' min..max.
2. The train loop: dronerl_amd.train.train with network_type "conv" (the
   default conv net) beside the dense (16, 16) net, at train_jax.py's defaults
   (num_envs 1, 1000 steps) and at 65,536 envs, twice each, in obs/s.
3. --trace-workload runs only 200 learner calls (default net, batch 8): the
   workload of a `rocprofv3 --kernel-trace --stats` run of its own, whose
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

AGENT5 = ({"out_channels": 4, "kernel_size": 3, "stride": 1, "padding": 1},)
TRAIN_JAX_CONV = ({"out_channels": 8, "kernel_size": 3, "stride": 1, "padding": 1},)
NETS = {"agent5": (AGENT5, (8,)), "train_jax_default": (TRAIN_JAX_CONV, ())}


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


def filled_ring(cap=300):
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import ReplayBuffer, decode_policy_code
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), 64)  # 7x7 windows
    env.reset(seed=0)
    rb = ReplayBuffer(cap, 294, torch.device("cuda"), code_radius=3)
    cur, nxt = env.new_code(), env.new_code()
    env.get_code(out=cur)
    for t in range(5):
        acts = env.synth_actions(seed=9, step=t)
        rew, don = env.step(acts, code=nxt)
        rb.add_many(cur, acts, rew, nxt, don)
        cur, nxt = nxt, cur
    f32 = {"obs": decode_policy_code(rb.obs, 3), "next_obs": decode_policy_code(rb.next_obs, 3)}
    torch.cuda.synchronize()
    return rb, f32


def learner_of(conv, dense, batch):
    from dronerl_amd.dqn import ConvDQNLearner, ConvQNetwork, DQNHParams
    net = ConvQNetwork((7, 7, 6), conv, dense, generator=torch.Generator().manual_seed(0), input="code")
    return ConvDQNLearner(net, DQNHParams(batch=batch, num_steps=1000))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-steps", type=int, default=1000)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--stats-csv", default=None, help="a rocprofv3 --kernel-trace --stats kernel_stats CSV to record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_learn", "learn.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.stats_csv:  # record the per-launch split of a profiler run of its own beside the timings
        with open(args.out) as f:
            result = json.load(f)
        with open(args.stats_csv) as f:
            rows = [r for r in csv.DictReader(f) if "drl_" in (r.get("Name") or "")]
        result["kernel_trace"] = {"command": "rocprofv3 --kernel-trace --stats -- python tools/time_conv_learn.py "
                                             "--trace-workload", "calls_per_kernel": 200 + 10, "kernels": rows}
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({"wrote": args.out, "kernels": len(rows)}))
        return
    rb, f32 = filled_ring()
    if args.trace_workload:
        learner = learner_of(*NETS["train_jax_default"], 8)
        for _ in range(210):
            learner.train(rb)
        torch.cuda.synchronize()
        learner.check_errors()
        print(json.dumps({"learner_calls": 210}))
        return
    result = {"command": " ".join(["python", "tools/time_conv_learn.py", *sys.argv[1:]]), "iters": args.iters,
              "reps": args.reps, "device": torch.cuda.get_device_name(0), "learner_call": {}, "train_loop": {}}
    for name, (conv, dense) in NETS.items():
        for batch in (8, 64):
            learner = learner_of(conv, dense, batch)
            variants = {"device": lambda: learner.train(rb),
                        "torch": torch_step_of(conv, learner, rb, f32, batch)}
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
            print(f"{name} batch {batch}: learner call {r['device']['median_us']:.1f} us "
                  f"({r['device']['min_us']:.1f}..{r['device']['max_us']:.1f}), torch step "
                  f"{r['torch']['median_us']:.1f} us ({r['torch']['min_us']:.1f}..{r['torch']['max_us']:.1f})")
    if not args.skip_loop:
        from dronerl_amd import EnvParams
        from dronerl_amd.train import train
        p = EnvParams(n_drones=4, grid_size=9)  # train_jax.py's defaults
        for envs in (1, 65536):
            for kind, kw in (("conv", dict(network_type="conv")), ("dense_16_16", dict(hidden=(16, 16)))):
                train(p, envs, 20, **kw)  # (warm-up: code objects)
                rates = [train(p, envs, args.loop_steps, **kw).env_steps_per_s for _ in range(2)]
                result["train_loop"][f"{kind}_envs{envs}"] = {
                    "steps": args.loop_steps, "obs_per_s": rates,
                    "us_per_step": [envs / r * 1e6 for r in rates]}
                print(f"train loop {kind}, {envs} envs, {args.loop_steps} steps: "
                      + ", ".join(f"{r:.4g} obs/s ({envs / r * 1e6:.1f} us/step)" for r in rates))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
