#!/usr/bin/env python3
"""Time the wide dense nets (drl_widenet_*, HIP events), tools/time_conv_act.py's method.

1. The act at 65,536 envs with 7x7 windows, from the f32 observation and from
   the policy code: run_jax_sweep.py's 294-256-128-64-5 net through
   drl_widenet_act beside checkpoint.TorchQNetwork on `cuda` (forward + argmax
   on the same observations, in the same process), and the 294-128-64-5 net
   through drl_widenet_act beside drl_qnet_act f32 / the code4 act, which is
   where routing keeps that net.
2. --learner: the learner call (drl_widenet_dqn_train) of the sweep net at
   batches 8, 64 and 1024 on a filled 8192-slot code ring, beside
   drl_dqn_large_train on 294-128-64-5 (tools/time_large_learn.py's method).
3. --train: train.train's loop (env steps per second) at 1 env and at 65,536
   envs for hidden (256, 128, 64) beside (128, 64).

Each act / learner figure is the median of --reps repetitions of --iters
calls, the variants alternating inside a repetition; the spread is the
repetitions' min..max.  Writes one JSON file.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

SWEEP = (256, 128, 64)  # run_jax_sweep.py:26
BENCH = (128, 64)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(iters):
        fn(t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "spread_us": max(v) - min(v),
            "reps_us": v}


def alternate(variants, iters, reps, warm=10):
    for fn in variants.values():
        timed(fn, warm)
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    return {k: summary(v) for k, v in times.items()}


def line(name, r):
    return f"{name}: " + ", ".join(f"{k} {s['median_us']:.1f} us ({s['min_us']:.1f}..{s['max_us']:.1f})"
                                   for k, s in r.items() if isinstance(s, dict) and "median_us" in s)


def time_act(args, result):
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.checkpoint import Checkpoint, TorchQNetwork
    from dronerl_amd.dqn import QNetwork, WideQNetwork
    E = args.envs
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), E)  # 7x7 windows
    env.reset(seed=0)
    code = env.new_code()
    for t in range(4):
        _, _, obs = env.step(env.synth_actions(seed=1, step=t), obs_k=1, code=code)
    obs = obs.reshape(E, 294).contiguous()
    torch.cuda.synchronize()
    a = torch.zeros((E, 1), dtype=torch.int32, device="cuda")
    q = torch.empty((E, 5), device="cuda")
    acts = {}
    for name, hidden in (("256_128_64", SWEEP), ("128_64", BENCH)):
        wide = {inp: WideQNetwork(294, hidden, generator=torch.Generator().manual_seed(0), input=inp)
                for inp in ("obs", "code")}
        variants = {"wide_obs": lambda s: wide["obs"].act(obs, 0.0, step=s, actions=a),
                    "wide_code": lambda s: wide["code"].act(code, 0.0, step=s, actions=a)}
        t = {}
        for i, (w, b) in enumerate(zip(wide["obs"].weights, wide["obs"].biases)):
            t[f"network.dense_{i + 1}.weight"], t[f"network.dense_{i + 1}.bias"] = w.cpu().numpy(), b.cpu().numpy()
        tnet = TorchQNetwork(Checkpoint("dense", (7, 7, 6), (5,), hidden, (), t)).eval().cuda()

        def torch_act(_):
            with torch.no_grad():
                return tnet(obs).argmax(dim=1)

        variants["torch"] = torch_act
        narrow = {}
        if max(hidden) <= 128:  # the specialised acts this net is routed to
            narrow = {inp: QNetwork(294, hidden, generator=torch.Generator().manual_seed(0), precision="f32", input=inp)
                      for inp in ("obs", "code")}
            variants["qnet_f32_obs"] = lambda s: narrow["obs"].act(obs, 0.0, step=s, actions=a)
            variants["qnet_code"] = lambda s: narrow["code"].act(code, 0.0, step=s, actions=a)
        # the same answers first
        wide["obs"].act(obs, 0.0, actions=a, q_out=q)
        ta = torch_act(0)
        torch.cuda.synchronize()
        agree = float((ta.int() == a[:, 0]).float().mean())
        r = alternate(variants, args.iters, args.reps)
        r["greedy_agreement_with_torch"] = agree
        worst = max(r[k]["spread_us"] for k in ("torch", "wide_obs", "wide_code"))
        for k in ("wide_obs", "wide_code"):
            r[k]["faster_than_torch_by_us"] = r["torch"]["median_us"] - r[k]["median_us"]
            r[k]["faster_than_torch_beyond_spread"] = bool(r[k]["faster_than_torch_by_us"] > worst)
        if narrow:
            r["wide_obs"]["times_qnet_f32_obs"] = r["wide_obs"]["median_us"] / r["qnet_f32_obs"]["median_us"]
            r["wide_code"]["times_qnet_code"] = r["wide_code"]["median_us"] / r["qnet_code"]["median_us"]
        acts[name] = r
        print(line(f"act {name} at {E} envs", r) + f"; greedy agreement with torch {agree:.5f}", flush=True)
        for n in (*wide.values(), *narrow.values()):
            n.check_errors()
    result["act"] = {"envs": E, "nets": acts}


def time_learner(args, result):
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams, LargeBatchDQNLearner, QNetwork, ReplayBuffer, WideDQNLearner, WideQNetwork
    cap = 8192
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), cap)
    env.reset(seed=0)
    rb = ReplayBuffer(cap, 294, torch.device("cuda"), code_radius=3)
    cur, nxt = env.new_code(), env.new_code()
    env.get_code(out=cur)
    acts = env.synth_actions(seed=9, step=0)
    rew, don = env.step(acts, code=nxt)
    rb.add_many(cur, acts, rew, nxt, don)
    torch.cuda.synchronize()
    out = {}
    for batch in (8, 64, 1024):
        hp = DQNHParams(batch=batch, num_steps=1000)
        wide = WideDQNLearner(WideQNetwork(294, SWEEP, generator=torch.Generator().manual_seed(0), input="code"), hp)
        large = LargeBatchDQNLearner(QNetwork(294, BENCH, generator=torch.Generator().manual_seed(0), input="code"), hp)
        r = alternate({"wide_256_128_64": lambda _: wide.train(rb), "large_128_64": lambda _: large.train(rb)},
                      args.iters, args.reps, warm=20)
        wide.check_errors()
        large.check_errors()
        out[f"batch{batch}"] = r
        print(line(f"learner call batch {batch}", r), flush=True)
    result["learner_call"] = {"ring_slots": cap, "batches": out}


def time_train(args, result):
    from dronerl_amd import EnvParams
    from dronerl_amd.train import train
    out = {}
    for E, steps in ((1, 300), (args.envs, 100)):
        for name, hidden in (("256_128_64", SWEEP), ("128_64", BENCH)):
            train(EnvParams(), E, 20, hidden=hidden)  # (warm-up: code objects, allocations)
            rates = [train(EnvParams(), E, steps, hidden=hidden).env_steps_per_s for _ in range(3)]
            out[f"{name}_envs{E}"] = {"steps": steps, "env_steps_per_s": rates,
                                      "us_per_step": [E / r * 1e6 for r in rates]}
            print(f"train {name} at {E} envs: " + ", ".join(f"{E / r * 1e6:.1f}" for r in rates) + " us per step",
                  flush=True)
    result["train_loop"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--learner", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_nets", "act.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    result = {"command": " ".join(["python", "tools/time_wide_act.py", *sys.argv[1:]]), "iters": args.iters,
              "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    time_act(args, result)
    if args.learner:
        time_learner(args, result)
    if args.train:
        time_train(args, result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
