"""Multi-agent evaluation on the device (drone_evaluator.py:97-204).

The reference scores a submission by letting six Q-networks each drive one
drone of a 6-drone env for ten seeded episodes of 1000 steps, adding every
step's rewards into a float64 array.  Here all line-ups x seeds run as ONE batch
of envs: per step one ``drl_obs_code_all`` (every drone's policy code), one act
launch per distinct (drone, net, env range), one ``drl_step`` and one
``drl_score_add`` (the reference's float64 arithmetic, bit for bit).

    evaluate_lineups(params, lineups, seeds, num_steps)   -> scores f64 [L, S, n_drones]
    evaluate_submissions(paths, baselines=DIR)            -> DroneRacerEvaluator._evaluate per path

PyTorch is plumbing (device memory, the current stream); the windows, the
policies, the step and the scores are libdronerl.so's HIP kernels.  Video, S3
upload and the AIcrowd payload are out of scope.
"""
from __future__ import annotations

import ctypes
import os
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._native import check, lib
from .env import BatchedDeliveryDrones, _ptr, _stream
from .params import EnvParams

EPISODE_SEEDS = (845, 99, 65, 96, 85, 39, 51, 17, 52, 35)   # drone_evaluator.py:28
TOTAL_EPISODE_STEPS = 1000                                   # drone_evaluator.py:29
# drone_evaluator.py:106-121 (n_drones = the six participating agents), WindowedGridView(radius=3)
EVALUATOR_ENV_PARAMS = {'charge_reward': -0.1, 'crash_reward': -1, 'delivery_reward': 1, 'charge': 20, 'discharge': 10,
                        'drone_density': 0.05, 'dropzones_factor': 2, 'n_drones': 6, 'packets_factor': 3,
                        'pickup_reward': 0, 'rgb_render_rescale': 1.0, 'skyscrapers_factor': 3, 'stations_factor': 2}
EVALUATOR_RADIUS = 3
CODE_WINDOWS = (5, 7, 9)  # windows the code acts accept (drl_qnet_act_code, drl_convnet_act, drl_widenet_act)
_REWARD_KEYS = ("crash_reward", "charge_reward", "pickup_reward", "delivery_reward")  # compat._py_reward's order


# ------------------------------------------------------------------ host side --
def seed_words(seed: int) -> List[int]:
    """CPython's getstate() words (624 MT words + index) right after ``random.seed(seed)``."""
    return [int(w) for w in random.Random(seed).getstate()[1]]


def env_index(lineup: int, seed_idx: int, num_seeds: int) -> int:
    """Env of (line-up l, seed s) in the batch: l * S + s."""
    return lineup * num_seeds + seed_idx


def reward_doubles(params) -> Tuple[float, float, float, float]:
    """The configured (crash, charge, pickup, delivery) rewards as the doubles the reference adds.  Two that
    round to one f32 but differ as doubles cannot be told apart in the kernel's f32 rewards: ValueError."""
    get = (lambda k: params[k]) if isinstance(params, dict) else (lambda k: getattr(params, k))
    vals = tuple(float(get(k)) for k in _REWARD_KEYS)
    for i in range(4):
        for j in range(i + 1, 4):
            if np.float32(vals[i]) == np.float32(vals[j]) and vals[i] != vals[j]:
                raise ValueError(f"{_REWARD_KEYS[i]}={vals[i]!r} and {_REWARD_KEYS[j]}={vals[j]!r} round to the same "
                                 "float32 but differ as doubles: their scores cannot be told apart")
    return vals


def reward_to_double(r, doubles: Sequence[float]) -> float:
    """drl_score_add's map of one f32 reward (compat._py_reward as a double): the first of crash, charge,
    pickup, delivery whose f32 rounding equals it, else 0.0 for a zero reward, else the f32 widened."""
    r = np.float32(r)
    for v in doubles:
        if np.float32(v) == r:
            return float(v)
    return 0.0 if r == 0 else float(r)


def _agent_key(a):
    if isinstance(a, (str, os.PathLike)):
        return ("path", os.path.realpath(os.fspath(a)))
    return ("obj", id(a))


def plan_acts(lineups, num_seeds: int, n_drones: int, envs: Optional[range] = None):
    """The act launches of one step.  -> (agents, acts, any_random):

    agents: the distinct non-None agents in first-appearance order (a checkpoint path given twice, in whatever
    spelling, is one agent; other objects are told apart by identity);
    acts: [(drone, agent index, lo, hi)], one per distinct (drone, agent, contiguous env range): consecutive
    line-ups with the same agent at a drone index share a launch.  Envs are l * S + s; with ``envs`` (a rank's
    shard of the global envs) the ranges are clipped to it and made local;
    any_random: some drone of some (local) env is None.
    """
    S = int(num_seeds)
    total = len(lineups) * S
    envs = range(0, total) if envs is None else envs
    agents, index, acts, any_random = [], {}, [], False
    for lu in lineups:
        if len(lu) != n_drones:
            raise ValueError(f"a line-up needs one agent per drone index ({n_drones}), got {len(lu)}")
    for d in range(n_drones):
        run = None  # (agent index or None, first line-up)
        for li in range(len(lineups) + 1):
            a = lineups[li][d] if li < len(lineups) else None
            key = None
            if li < len(lineups) and a is not None:
                k = _agent_key(a)
                if k not in index:
                    index[k] = len(agents)
                    agents.append(a)
                key = index[k]
            if run is not None and (li == len(lineups) or key != run[0]):
                lo, hi = max(run[1] * S, envs.start), min(li * S, envs.stop)
                if lo < hi:
                    if run[0] is None:
                        any_random = True
                    else:
                        acts.append((d, run[0], lo - envs.start, hi - envs.start))
                run = None
            if run is None and li < len(lineups):
                run = (key, li)
    return agents, acts, any_random


def build_agent(path, window_radius: int, device=None):
    """A checkpoint as a device net for a (2r+1)-wide window: policy-code input where the code acts accept the
    window (radius 2..4), f32 observation rows otherwise."""
    from .checkpoint import qnet_class_of, read_checkpoint, to_qnet
    from .dqn import QNetwork
    ck = read_checkpoint(os.fspath(path))
    W = 2 * window_radius + 1
    if tuple(ck.obs_shape) != (W, W, 6):
        raise ValueError(f"{path}: trained on observations {tuple(ck.obs_shape)}, the env's windows are {(W, W, 6)}")
    if int(ck.action_shape[0]) != 5:
        raise ValueError(f"{path}: {ck.action_shape[0]} actions, the env has 5")
    inp = "code" if W in CODE_WINDOWS else "obs"
    if ck.network_type == "dense" and inp == "code" and qnet_class_of(ck.dense_layers) is QNetwork:
        net = QNetwork(W * W * 6, ck.dense_layers, 5, device=device, input="code")
        n = len(ck.dense_layers) + 1
        net.load([torch.from_numpy(np.array(ck.tensors[f"network.dense_{i + 1}.weight"])) for i in range(n)],
                 [torch.from_numpy(np.array(ck.tensors[f"network.dense_{i + 1}.bias"])) for i in range(n)])
        return net
    return to_qnet(ck, device=device, input=inp)


# ---------------------------------------------------------------- device side --
def obs_code_all(env: BatchedDeliveryDrones, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Every drone's policy code, uint8 [n_drones, E, policy_code_bytes] (drl_obs_code_all): block d holds what
    ``get_code()`` would write with drone index d in index 0's place."""
    shape = (env.n_drones, env.num_envs, env.policy_code_bytes)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=env.device)
    env._check_out(out, torch.uint8, shape, "codes")
    s = env.state.c()
    check(lib().drl_obs_code_all(ctypes.byref(env._cp), ctypes.byref(s), _ptr(out), _stream(env.device)),
          "drl_obs_code_all")
    return out


def score_add(rewards: torch.Tensor, scores: torch.Tensor, doubles: Sequence[float]) -> torch.Tensor:
    """scores f64 [E, N] += the doubles of one step's f32 rewards [E, N] (drl_score_add; ``doubles`` from
    ``reward_doubles``)."""
    if (rewards.dtype != torch.float32 or scores.dtype != torch.float64 or rewards.dim() != 2
            or rewards.shape != scores.shape or rewards.device != scores.device or rewards.device.type != "cuda"
            or not rewards.is_contiguous() or not scores.is_contiguous()):
        raise ValueError("rewards must be float32 [E, N] and scores float64 [E, N], contiguous, on one GPU")
    c, g, p, d = (float(v) for v in doubles)
    check(lib().drl_score_add(_ptr(rewards), rewards.shape[0], rewards.shape[1], c, g, p, d, _ptr(scores),
                              _stream(rewards.device)), "drl_score_add")
    return scores


def _is_net(a) -> bool:
    from .dqn import ConvQNetwork, QNetwork, WideQNetwork
    return isinstance(a, (QNetwork, WideQNetwork, ConvQNetwork))


def evaluate_lineups(params: EnvParams, lineups, seeds: Sequence[int], num_steps: int, device=None,
                     action_seed: int = 0, record_actions: bool = False, rank: int = 0, world: int = 1):
    """Score line-ups of agents over seeded episodes: float64 [len(lineups), len(seeds), n_drones] (numpy).

    A line-up is a list of n_drones agents, one per drone index: a device net (QNetwork / WideQNetwork /
    ConvQNetwork, input "code" or "obs"), a checkpoint path (``build_agent``; the same path is loaded once),
    None (a uniformly random drone: its column of ``synth_actions(action_seed, t)`` at the batch's env index)
    or a host callable ``f(windows f32 [n, W, W, 6]) -> int [n]``.  Nets act greedily (epsilon 0).

    Env l * S + s runs line-up l from ``set_seed(env, seeds[s]); env.reset()`` (any integer seed) and adds its
    rewards exactly as the reference's ``episode_scores += step_score``.  record_actions: also return the
    actions, int32 [num_steps, L * S, n_drones].  world > 1: the envs are sharded over ranks
    (distributed.shard_episodes) and the tables all-reduced, as distributed.evaluate_sharded does.
    """
    from .distributed import allreduce_sum, shard_episodes
    from .dqn import decode_policy_code
    N, S, L = params.n_drones, len(seeds), len(lineups)
    total = L * S
    if total == 0:
        raise ValueError("need at least one line-up and one seed")
    doubles = reward_doubles(params)
    envs = shard_episodes(total, rank, world)
    agents, acts, any_random = plan_acts(lineups, S, N, envs)
    E = len(envs)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    table = torch.zeros((total, N), dtype=torch.float64, device=dev)
    rec = torch.zeros((num_steps, total, N), dtype=torch.int32, device=dev) if record_actions else None
    nets = []
    if E:
        env = BatchedDeliveryDrones(params, E, device=dev, env_offset=envs.start)
        dev = env.device
        R, W = params.window_radius, 2 * params.window_radius + 1
        used = {ai for _, ai, _, _ in acts}
        built = {}
        for ai, a in enumerate(agents):
            if ai not in used:
                continue
            if isinstance(a, (str, os.PathLike)):
                a = build_agent(a, R, dev)
            elif _is_net(a):
                if a.in_features != W * W * 6 or a.n_actions != 5:
                    raise ValueError(f"a net of {a.in_features} inputs / {a.n_actions} actions cannot drive a "
                                     f"{W}x{W} window with 5 actions")
            elif not callable(a):
                raise ValueError(f"agent {a!r}: a device net, a checkpoint path, None or a callable")
            built[ai] = a
        nets = [a for a in built.values() if _is_net(a)]
        words = {}
        for s in seeds:
            if s not in words:
                words[s] = seed_words(s)
        env.set_mt_words(np.array([words[seeds[g % S]] for g in envs], dtype=np.int64))
        env.reset(seed=None)
        codes = obs_code_all(env)
        # (one spare row: a drone's act writes column 0 of the [n, N] view that starts at its own column)
        flat = torch.zeros(E * N + N, dtype=torch.int32, device=dev)
        actions = flat[:E * N].view(E, N)
        rewards = torch.empty((E, N), dtype=torch.float32, device=dev)
        dones = torch.empty((E, N), dtype=torch.uint8, device=dev)
        scores = torch.zeros((E, N), dtype=torch.float64, device=dev)
        need_obs = max((hi - lo for _, ai, lo, hi in acts if not (_is_net(built[ai]) and built[ai].input == "code")),
                       default=0)
        obs = torch.empty((need_obs, W * W * 6), dtype=torch.float32, device=dev) if need_obs else None
        for t in range(num_steps):
            obs_code_all(env, codes)
            if any_random:
                env.synth_actions(action_seed, t, out=actions)
            for d, ai, lo, hi in acts:
                a, n = built[ai], hi - lo
                rows = codes[d, lo:hi]
                if _is_net(a):
                    col = flat[lo * N + d: lo * N + d + n * N].view(n, N)
                    a.act(rows if a.input == "code" else decode_policy_code(rows, R, out=obs[:n]), 0.0, actions=col)
                else:
                    win = decode_policy_code(rows, R, out=obs[:n]).cpu().numpy().reshape(n, W, W, 6)
                    chosen = np.asarray(a(win)).astype(np.int32).reshape(n)
                    actions[lo:hi, d] = torch.from_numpy(chosen).to(dev)
            if rec is not None:
                rec[t, envs.start:envs.stop] = actions
            env.step(actions, rewards=rewards, dones=dones)
            score_add(rewards, scores, doubles)
        env.check_errors()
        for net in nets:
            net.check_errors()
        table[envs.start:envs.stop] = scores
    if world > 1:
        allreduce_sum(table)
        if rec is not None:
            allreduce_sum(rec)
    out = table.cpu().numpy().reshape(L, S, N)
    if record_actions:
        return out, rec.cpu().numpy()
    return out


# ------------------------------------------------------- the reference evaluator --
def baseline_paths(baselines) -> dict:
    """{"baseline-i": path}: from a directory holding dqn-agent-1..5.safetensors (drone_evaluator.py:30-36),
    a sequence of paths, or such a dict as is."""
    if isinstance(baselines, dict):
        return {str(k): os.fspath(v) for k, v in baselines.items()}
    if isinstance(baselines, (str, os.PathLike)):
        return {f"baseline-{i}": os.path.join(os.fspath(baselines), f"dqn-agent-{i}.safetensors") for i in range(1, 6)}
    return {f"baseline-{i + 1}": os.fspath(p) for i, p in enumerate(baselines)}


def evaluate_submissions(paths: Sequence, baselines="sample_models", seeds: Sequence[int] = EPISODE_SEEDS,
                         num_steps: int = TOTAL_EPISODE_STEPS, params: Optional[EnvParams] = None, device=None,
                         record_actions: bool = False, rank: int = 0, world: int = 1) -> List[dict]:
    """DroneRacerEvaluator._evaluate for every submission, all in one batch of envs.

    Each path meets the baselines in a line-up sorted by agent name ("YOU" sorts before "baseline-*": the
    submission is drone 0).  params: the evaluator's env by default (6 drones at density 0.05: side 11, radius
    3).  -> per path {"path", "scores" f64 [episodes, agents], "score", "score_secondary"} (numpy's mean / std
    over episodes of drone 0, drone_evaluator.py:199-204) and, with record_actions, "actions" int32
    [num_steps, episodes, agents].
    """
    base = baseline_paths(baselines)
    if params is None:
        cfg = dict(EVALUATOR_ENV_PARAMS)
        cfg["n_drones"] = len(base) + 1
        params = EnvParams.from_torch_config(cfg, window_radius=EVALUATOR_RADIUS)
    if params.n_drones != len(base) + 1:
        raise ValueError(f"{len(base)} baselines and the submission need n_drones = {len(base) + 1}")
    lineups = []
    for p in paths:
        named = dict(base)
        named["YOU"] = os.fspath(p)
        lineups.append([named[k] for k in sorted(named)])
    you = sorted(list(base) + ["YOU"]).index("YOU")
    out = evaluate_lineups(params, lineups, list(seeds), num_steps, device=device, record_actions=record_actions,
                           rank=rank, world=world)
    scores, acts = out if record_actions else (out, None)
    S = len(seeds)
    results = []
    for i, p in enumerate(paths):
        tab = scores[i]
        r = {"path": os.fspath(p), "scores": tab, "score": float(tab.mean(axis=0)[you]),
             "score_secondary": float(tab.std(axis=0)[you])}
        if acts is not None:
            r["actions"] = acts[:, i * S:(i + 1) * S]
        results.append(r)
    return results
