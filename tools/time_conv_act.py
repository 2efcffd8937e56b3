#!/usr/bin/env python3
"""Time the conv Q-network act (drl_convnet_act, HIP events) against the only
other way to run these nets on the GPU: checkpoint.TorchQNetwork moved to
cuda, forward + argmax on the same observations, in the same process.

Nets: the reference's sample_models/dqn-agent-5 (conv 6->4 k3 p1, dense 8) and
train_jax.py's default conv net (conv 6->8 k3 p1, the flatten straight into
the Q head), at 65,536 envs with 7x7 windows, from the f32 observation and
from the policy code.  Each figure is the median of --reps repetitions of
--iters launches, the variants alternating inside a repetition; the spread is
the repetitions' min..max.  The read floor is the input's bytes (1,176 B of
observation or 128 B of code per env) over the 6.79 TB/s measured read peak
(README).  Writes one JSON file.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

READ_PEAK = 6.79e12  # B/s, README (drl_hbm_probe's read form)
TRAIN_JAX_CONV = ({"out_channels": 8, "kernel_size": 3, "stride": 1, "padding": 1},)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_act", "act.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.checkpoint import Checkpoint, TorchQNetwork, read_checkpoint, to_qnet
    from dronerl_amd.dqn import ConvQNetwork
    E = args.envs
    env = BatchedDeliveryDrones(EnvParams(n_drones=8, grid_size=16), E)  # 7x7 windows
    env.reset(seed=0)
    code = env.new_code()
    for t in range(4):
        _, _, obs = env.step(env.synth_actions(seed=1, step=t), obs_k=1, code=code)
    obs = obs.reshape(E, 7, 7, 6).contiguous()
    torch.cuda.synchronize()

    ck5 = read_checkpoint(os.path.join(REPO, "tests", "golden", "sample_models", "dqn-agent-5.safetensors"))
    dflt = ConvQNetwork((7, 7, 6), TRAIN_JAX_CONV, (), generator=torch.Generator().manual_seed(0))
    t = {"network.conv2d_1.weight": dflt.conv_weights[0], "network.conv2d_1.bias": dflt.conv_biases[0],
         "network.dense_1.weight": dflt.weights[0], "network.dense_1.bias": dflt.biases[0]}
    ckd = Checkpoint("conv", (7, 7, 6), (5,), (), TRAIN_JAX_CONV, {k: v.cpu().numpy() for k, v in t.items()})
    result = {"envs": E, "iters": args.iters, "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "read_peak_TBps": READ_PEAK / 1e12, "nets": {}}
    for name, ck in (("agent5", ck5), ("train_jax_default", ckd)):
        nets = {inp: to_qnet(ck, device="cuda", input=inp) for inp in ("obs", "code")}
        tnet = TorchQNetwork(ck).eval().cuda()
        a = torch.zeros((E, 1), dtype=torch.int32, device="cuda")
        q = torch.empty((E, 5), device="cuda")

        def torch_act(_):
            with torch.no_grad():
                return tnet(obs).argmax(dim=1)

        variants = {"obs": lambda s: nets["obs"].act(obs, 0.0, step=s, actions=a),
                    "code": lambda s: nets["code"].act(code, 0.0, step=s, actions=a),
                    "torch": torch_act}
        # the same answers first (and the warm-up of every variant: code objects, the library's algorithm choice)
        nets["obs"].act(obs, 0.0, actions=a, q_out=q)
        ta = torch_act(0)
        torch.cuda.synchronize()
        agree = float((ta.int() == a[:, 0]).float().mean())
        for fn in variants.values():
            timed(fn, 10)
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, args.iters))
        r = {k: summary(v) for k, v in times.items()}
        r["greedy_agreement_with_torch"] = agree
        r["read_floor_us"] = {"obs": E * 1176 / READ_PEAK * 1e6, "code": E * 128 / READ_PEAK * 1e6}
        worst = max(r["torch"]["spread_us"], r["obs"]["spread_us"], r["code"]["spread_us"])
        for k in ("obs", "code"):
            r[k]["times_read_floor"] = r[k]["median_us"] / r["read_floor_us"][k]
            r[k]["faster_than_torch_by_us"] = r["torch"]["median_us"] - r[k]["median_us"]
            r[k]["faster_than_torch_beyond_spread"] = bool(r[k]["faster_than_torch_by_us"] > worst)
        result["nets"][name] = r
        print(f"{name}: act obs {r['obs']['median_us']:.1f} us ({r['obs']['min_us']:.1f}..{r['obs']['max_us']:.1f}), "
              f"code {r['code']['median_us']:.1f} us ({r['code']['min_us']:.1f}..{r['code']['max_us']:.1f}), "
              f"torch forward + argmax {r['torch']['median_us']:.1f} us "
              f"({r['torch']['min_us']:.1f}..{r['torch']['max_us']:.1f}); floors {r['read_floor_us']['obs']:.1f} / "
              f"{r['read_floor_us']['code']:.2f} us; greedy agreement {agree:.5f}")
        for n in nets.values():
            n.check_errors()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
