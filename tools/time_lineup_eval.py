#!/usr/bin/env python3
"""Time the multi-agent evaluator (dronerl_amd.evaluator; HIP events, tools/time_wide_act.py's method).

(a) Wall time of the reference line-up: evaluate_submissions on submission 1 (10 episodes x 1000 steps, one batch
    of 10 envs) beside tests/test_evaluator_parity.run_compat(1) in the same process -- one env at a time through
    dronerl_amd.compat, the only way to evaluate before.
(b) One evaluation step at 4,096 and 65,536 envs (side 11, 6 drones, radius 3; the six sample nets of the
    reference line-up), split into drl_obs_code_all, the six code acts, the env step and drl_score_add, beside the
    f32 route through the existing kernels: get_obs(6) and the six obs acts (obs_stride = 6 * 294, action_stride =
    6).  Each figure is the median of --reps repetitions of --iters calls, the variants alternating inside a
    repetition; the spread is the repetitions' min..max.  The code kernel's bytes (per env 64 B of ground and 24 B
    of records read, 6 x 128 B written) are held against bench.py's measured copy peak.
(c) Whether the device nets' scores over the full 1000 steps equal the golden table for all five submissions
    (recorded, not asserted anywhere).

Writes one JSON file.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
MODELS = os.path.join(GOLD, "sample_models")


def model(i):
    return os.path.join(MODELS, f"dqn-agent-{i}.safetensors")


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


def wall(fn, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out), "runs_s": out}


def time_reference_lineup(args, result):
    from dronerl_amd import evaluator as ev
    golden = np.load(os.path.join(GOLD, "evaluator_scores.npz"))["scores"]
    ev.evaluate_submissions([model(1)], baselines=MODELS, num_steps=20)  # (warm-up: code objects, allocations)
    batched = wall(lambda: ev.evaluate_submissions([model(1)], baselines=MODELS), 3)
    r = {"episodes": 10, "steps": 1000, "evaluate_submissions": batched}
    if not args.no_compat:
        import test_evaluator_parity as tp
        r["run_compat"] = wall(lambda: tp.run_compat(1), 1)
        r["speedup"] = r["run_compat"]["median_s"] / batched["median_s"]
    res = ev.evaluate_submissions([model(i) for i in range(1, 6)], baselines=MODELS)
    r["device_scores_equal_golden"] = {str(i + 1): bool(np.array_equal(res[i]["scores"], golden[i])) for i in range(5)}
    r["device_score"] = {str(i + 1): [res[i]["score"], res[i]["score_secondary"]] for i in range(5)}
    result["reference_lineup"] = r
    print(json.dumps({k: v for k, v in r.items() if k != "device_score"}), flush=True)


def time_step(args, result, copy_peak):
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd import evaluator as ev
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    params = EnvParams.from_torch_config(ev.EVALUATOR_ENV_PARAMS, window_radius=3)
    N, doubles = 6, ev.reward_doubles(params)
    subs = (1, 1, 2, 3, 4, 5)  # submission 1's line-up: YOU, baseline-1..5
    code_nets = {i: ev.build_agent(model(i), 3, "cuda") for i in set(subs)}
    obs_nets = {i: to_qnet(read_checkpoint(model(i)), device="cuda", input="obs") for i in set(subs)}
    out = {}
    for E in args.envs:
        env = BatchedDeliveryDrones(params, E)
        env.reset(seed=0)
        codes = ev.obs_code_all(env)
        obs = env.get_obs(N)
        flat = torch.zeros(E * N + N, dtype=torch.int32, device="cuda")
        actions = flat[:E * N].view(E, N)
        cols = [flat[d:d + E * N].view(E, N) for d in range(N)]
        rewards = torch.empty((E, N), dtype=torch.float32, device="cuda")
        dones = torch.empty((E, N), dtype=torch.uint8, device="cuda")
        scores = torch.zeros((E, N), dtype=torch.float64, device="cuda")
        ob = obs.reshape(E, N, -1)

        def acts_code(_):
            for d, i in enumerate(subs):
                code_nets[i].act(codes[d], 0.0, actions=cols[d])

        def acts_obs(_):
            for d, i in enumerate(subs):
                obs_nets[i].act(ob[:, d], 0.0, actions=cols[d])

        def step(_):
            env.step(actions, rewards=rewards, dones=dones)

        def route_code(t):
            ev.obs_code_all(env, codes)
            acts_code(t)
            step(t)
            ev.score_add(rewards, scores, doubles)

        def route_obs(t):
            env.get_obs(N, out=obs)
            acts_obs(t)
            step(t)
            ev.score_add(rewards, scores, doubles)

        r = alternate({"obs_code_all": lambda _: ev.obs_code_all(env, codes), "acts_code": acts_code,
                       "get_obs_f32": lambda _: env.get_obs(N, out=obs), "acts_obs_f32": acts_obs, "env_step": step,
                       "score_add": lambda _: ev.score_add(rewards, scores, doubles),
                       "step_code_route": route_code, "step_f32_route": route_obs}, args.iters, args.reps)
        env.check_errors()
        for n in (*code_nets.values(), *obs_nets.values()):
            n.check_errors()
        c, f = r["step_code_route"], r["step_f32_route"]
        worst = max(c["spread_us"], f["spread_us"])
        r["code_route_faster_by_us"] = f["median_us"] - c["median_us"]
        r["code_route_faster_beyond_spread"] = bool(f["median_us"] - c["median_us"] > worst)
        nbytes = E * (params.layout().ground_stride + 4 * N + N * env.policy_code_bytes)
        r["obs_code_all_bytes"] = nbytes
        r["obs_code_all_GBs"] = nbytes / r["obs_code_all"]["median_us"] / 1e3
        if copy_peak:
            r["obs_code_all_vs_copy_peak"] = r["obs_code_all_GBs"] / copy_peak["copy_GBs"]
        out[str(E)] = r
        print(f"{E} envs: " + ", ".join(f"{k} {s['median_us']:.1f} us ({s['min_us']:.1f}..{s['max_us']:.1f})"
                                        for k, s in r.items() if isinstance(s, dict)), flush=True)
        del env, codes, obs, ob
        torch.cuda.empty_cache()
    result["step"] = {"side": params.side, "n_drones": N, "radius": 3, "envs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-compat", action="store_true", help="skip the one-env-at-a-time compat run (about a minute)")
    ap.add_argument("--no-copy-peak", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lineup_eval", "eval.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    result = {"command": " ".join(["python", "tools/time_lineup_eval.py", *sys.argv[1:]]), "iters": args.iters,
              "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    copy_peak = None
    if not args.no_copy_peak:
        import bench
        copy_peak = bench.measure_copy_peak(torch.device("cuda", 0))
        result["copy_peak"] = copy_peak
    time_step(args, result, copy_peak)
    time_reference_lineup(args, result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
