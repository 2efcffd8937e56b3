"""A league: several DQN agents trained against each other in shared envs
(include/dronerl.h drl_league_*; dronerl_amd/csrc/league/).

Reference: torch_impl/helpers/rl_helpers.py:21-65, MultiAgentTrainer.train --
every drone index has its own agent, all agents act, the env steps once and
each agent learns from its own drone's transition; train_torch.py:107-122 and
create_baselines.py:79-101 run the same loop with the other drones random.
`evaluate_lineups` is the other half (DroneRacerEvaluator._evaluate): a net
trained here meets, in training, the line-up it is scored in.

One batch of E envs with N drones each and K learners, 1 <= K <= N: learner
k drives drone INDEX k of every env.  Each learner is exactly a population
member (`PopulationDQN` with members = K: its own parameters, Adam state,
counters, hyperparameter record and replay ring; oracle/dqn_learner.py's
arithmetic bit for bit), so `drl_pop_train` and the ring layout are reused
unchanged.  Drones K..N-1 are each random (their column of
`synth_actions(action_seed, t)`) or a fixed net acting greedily on its block
of the code, exactly as the evaluator drives it.

Learner k's exploration draw in env i is
explore_draw(seed + k, step, env_offset + i, n_actions, epsilon_k): with
k = 0 the population's stream, so a league of one learner with the other
drones random is `train_population` with one member, bit for bit.

Conv learners (`ConvLeagueDQN`, train_league(network_type="conv"),
`python -m dronerl_amd.conv_league`): each learner is a ConvPopulationDQN
member and everything above holds with the conv population in the dense
one's place; the act is drl_convleague_act (dronerl_amd/csrc/convleague/).
One architecture per league: dense and conv learners do not mix.

    train_league(params, learners, num_envs, num_steps, opponents={4: path}) -> LeagueResult
    evaluate_league(result)                                     -> the greedy table
    python -m dronerl_amd.league --learners 2 --opponents a.safetensors b.safetensors ...
"""
from __future__ import annotations

import ctypes
import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import torch

from .dqn import DQNHParams, DrlReplay, DrlWidenetDesc, _check, _on, _stream, _vp
from .params import EnvParams
from .population import ConvPopulationDQN, PopulationDQN, PopulationReplay, _bind_pop

U64 = 2 ** 64 - 1


class DrlLeagueActPlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("env_tile", "threads", "pass_units", "chunk_k", "ldx", "lda",
                                               "lds_bytes", "lds_limit")]


def _bind_league(L):
    if getattr(L, "_league_ready", False):
        return L
    _bind_pop(L)
    i32, i64, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    D, R = ctypes.POINTER(DrlWidenetDesc), ctypes.POINTER(DrlReplay)
    sig = {
        "drl_league_act_plan_query": [D, ctypes.POINTER(DrlLeagueActPlan)],
        "drl_league_act": [D, i32, i32, _vp, _vp, i64, i32, u64, u64, i64, _vp, i32, _vp, _vp],
        "drl_league_replay_add": [D, i32, R, i64, i64, _vp, _vp, _vp, _vp, _vp, i32, _vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = ctypes.c_int
    L._league_ready = True
    return L


def act_plan(desc: DrlWidenetDesc) -> dict:
    """The act kernel's tiling for a population description
    (drl_league_act_plan_query): env_tile, threads, pass_units, chunk_k, the
    LDS row strides and bytes, the limit they stay within."""
    from ._native import lib
    from .dqn import _bind
    L = _bind_league(_bind(lib()))
    p = DrlLeagueActPlan()
    if L.drl_league_act_plan_query(ctypes.byref(desc), ctypes.byref(p)):
        raise ValueError(L.drl_last_error().decode())
    return {n: int(getattr(p, n)) for n, _ in DrlLeagueActPlan._fields_}


class LeagueReplay(PopulationReplay):
    """K replay rings in one allocation, ring k fed by drone index k of the
    shared envs (drl_league_replay_add): env i lands in slot
    (cursor + i) % capacity of every ring, and an add larger than the ring
    keeps its last `capacity` envs.  The layout, cursor and size are
    PopulationReplay's."""

    def __init__(self, members: int, capacity: int, window_radius: int, device=None):
        super().__init__(members, capacity, window_radius, device=device)
        _bind_league(self.L)

    def add(self, codes_prev: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, codes: torch.Tensor,
            dones: torch.Tensor):
        """codes_prev / codes: uint8 [n_drones, E, code_bytes]
        (evaluator.obs_code_all: what the act read, what the step left);
        actions i32, rewards f32, dones u8 [E, n_drones] (ring k takes column
        k)."""
        dev = self.obs.device
        for t, dt, name in ((codes_prev, torch.uint8, "codes_prev"), (codes, torch.uint8, "codes"),
                            (actions, torch.int32, "actions"), (rewards, torch.float32, "rewards"),
                            (dones, torch.uint8, "dones")):
            _on(t, dev, dt, name)
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        if codes.dim() != 3 or codes.shape != codes_prev.shape or codes.shape[2] != self.code_bytes:
            raise ValueError(f"codes and codes_prev must be uint8 [n_drones, E, {self.code_bytes}]")
        N, E = int(codes.shape[0]), int(codes.shape[1])
        for t, name in ((actions, "actions"), (rewards, "rewards"), (dones, "dones")):
            if tuple(t.shape) != (E, N):
                raise ValueError(f"{name} must be [{E}, {N}] (envs by drones)")
        _check(self.L, self.L.drl_league_replay_add(ctypes.byref(self.desc), self.members, ctypes.byref(self._c),
                                                    self.cursor, E, _vp(codes_prev.data_ptr()),
                                                    _vp(codes.data_ptr()), _vp(actions.data_ptr()),
                                                    _vp(rewards.data_ptr()), _vp(dones.data_ptr()), N,
                                                    _stream(dev)))
        self.cursor = (self.cursor + E) % self.capacity
        self.size = min(self.size + E, self.capacity)


DOUBLE_LEAGUE_REFUSAL = ("double_dqn: a league's learners (LeagueDQN, ConvLeagueDQN) train the max rule only; Double "
                         "DQN is implemented for single dense agents and dense populations")


class LeagueDQN(PopulationDQN):
    """K learners over the same E envs, learner k on drone index k: a
    PopulationDQN with members = K and envs_per_member = E whose act reads
    block k of every drone's code and writes column k of the action matrix
    (drl_league_act).  `train`, `member_net`, `save`, `params`, `counters`
    and `sample_slots` are the population's."""

    _double_refusal = DOUBLE_LEAGUE_REFUSAL

    def __init__(self, in_features: int, hidden: Sequence[int], hps: Sequence[DQNHParams], num_envs: int, **kw):
        super().__init__(in_features, hidden, hps, num_envs, **kw)
        _bind_league(self.L)

    @property
    def act_plan(self) -> dict:
        return act_plan(self.desc)

    def act(self, codes: torch.Tensor, step: int, seed: int = 0, env_offset: int = 0,
            actions: Optional[torch.Tensor] = None, greedy: bool = False,
            q: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Columns 0..K-1 of actions [E, n_drones] (no other column is
        written): learner k's epsilon-greedy action of env i from its online
        net on codes[k, i] and its device epsilon (greedy: no exploration,
        whatever epsilon holds), the draw keyed on (seed + k, step,
        env_offset + i).  codes: uint8 [n_drones, E, code_bytes]
        (evaluator.obs_code_all).  q: float32 [K, E, n_actions]."""
        K, E = self.members, self.E
        _on(codes, self.device, torch.uint8, "codes")
        if codes.dim() != 3 or tuple(codes.shape[1:]) != (E, self.code_bytes) or not codes.is_contiguous():
            raise ValueError(f"codes must be a contiguous uint8 [n_drones, {E}, {self.code_bytes}] tensor")
        N = int(codes.shape[0])
        if actions is None:
            actions = torch.zeros((E, N), dtype=torch.int32, device=self.device)
        _on(actions, self.device, torch.int32, "actions")
        if tuple(actions.shape) != (E, N) or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous int32 [{E}, {N}] tensor")
        if q is not None:
            _on(q, self.device, torch.float32, "q")
            if tuple(q.shape) != (K, E, self.n_actions) or not q.is_contiguous():
                raise ValueError(f"q must be a contiguous float32 [{K}, {E}, {self.n_actions}] tensor")
        _check(self.L, self.L.drl_league_act(
            ctypes.byref(self.desc), K, self.max_batch, _vp(self.block.data_ptr()), _vp(codes.data_ptr()), E,
            int(bool(greedy)), int(seed) & U64, int(step), int(env_offset), _vp(actions.data_ptr()), N,
            None if q is None else _vp(q.data_ptr()), _stream(self.device)))
        return actions


class DrlConvLeagueActPlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("env_tile", "threads", "row_words", "lds_bytes", "lds_limit")]


def _bind_convleague(L):
    if getattr(L, "_convleague_ready", False):
        return L
    from .dqn import DrlConvnetDesc
    _bind_league(L)
    i32, i64, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    D = ctypes.POINTER(DrlConvnetDesc)
    sig = {
        "drl_convleague_act_plan_query": [D, ctypes.POINTER(DrlConvLeagueActPlan)],
        "drl_convleague_act": [D, i32, i32, _vp, _vp, i64, i32, u64, u64, i64, _vp, i32, _vp, _vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = ctypes.c_int
    L._convleague_ready = True
    return L


def conv_act_plan(desc) -> dict:
    """The conv league act's tiling for a conv population description
    (drl_convleague_act_plan_query): env_tile, threads, the LDS words of an
    env's forward-only row, the launch's LDS bytes and their limit."""
    from ._native import lib
    from .dqn import _bind
    L = _bind_convleague(_bind(lib()))
    p = DrlConvLeagueActPlan()
    if L.drl_convleague_act_plan_query(ctypes.byref(desc), ctypes.byref(p)):
        raise ValueError(L.drl_last_error().decode())
    return {n: int(getattr(p, n)) for n, _ in DrlConvLeagueActPlan._fields_}


class ConvLeagueDQN(ConvPopulationDQN):
    """K conv learners over the same E envs, learner k on drone index k: a
    ConvPopulationDQN with members = K and envs_per_member = E whose act is
    LeagueDQN.act's (drl_convleague_act: block k of every drone's code in,
    column k of the action matrix out, T envs of a learner per workgroup so
    that a fetched weight serves them all).  Its Q is drl_convpop_act's bit
    for bit.  `train`, `member_net`, `save`, `params`, `counters` and
    `sample_slots` are the conv population's."""

    _double_refusal = DOUBLE_LEAGUE_REFUSAL

    def __init__(self, obs_shape, conv_layers, dense_layers: Sequence[int], hps: Sequence[DQNHParams],
                 num_envs: int, **kw):
        super().__init__(obs_shape, conv_layers, dense_layers, hps, num_envs, **kw)
        _bind_convleague(self.L)

    @property
    def act_plan(self) -> dict:
        return conv_act_plan(self.desc)

    def act(self, codes: torch.Tensor, step: int, seed: int = 0, env_offset: int = 0,
            actions: Optional[torch.Tensor] = None, greedy: bool = False,
            q: Optional[torch.Tensor] = None) -> torch.Tensor:
        """LeagueDQN.act's arguments, checks and result."""
        K, E = self.members, self.E
        _on(codes, self.device, torch.uint8, "codes")
        if codes.dim() != 3 or tuple(codes.shape[1:]) != (E, self.code_bytes) or not codes.is_contiguous():
            raise ValueError(f"codes must be a contiguous uint8 [n_drones, {E}, {self.code_bytes}] tensor")
        N = int(codes.shape[0])
        if actions is None:
            actions = torch.zeros((E, N), dtype=torch.int32, device=self.device)
        _on(actions, self.device, torch.int32, "actions")
        if tuple(actions.shape) != (E, N) or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous int32 [{E}, {N}] tensor")
        if q is not None:
            _on(q, self.device, torch.float32, "q")
            if tuple(q.shape) != (K, E, self.n_actions) or not q.is_contiguous():
                raise ValueError(f"q must be a contiguous float32 [{K}, {E}, {self.n_actions}] tensor")
        _check(self.L, self.L.drl_convleague_act(
            ctypes.byref(self.desc), K, self.max_batch, _vp(self.block.data_ptr()), _vp(codes.data_ptr()), E,
            int(bool(greedy)), int(seed) & U64, int(step), int(env_offset), _vp(actions.data_ptr()), N,
            None if q is None else _vp(q.data_ptr()), _stream(self.device)))
        return actions


def resolve_opponents(opponents, learners: int, params: EnvParams, device=None) -> Dict[int, object]:
    """{drone index: device net} for the fixed opponents; an index that is
    missing or maps to None is a random drone.  A path is loaded as the
    evaluator loads it (evaluator.build_agent)."""
    from .evaluator import _is_net, build_agent
    N, W = params.n_drones, 2 * params.window_radius + 1
    out = {}
    for d, a in sorted((opponents or {}).items()):
        d = int(d)
        if d < learners:
            raise ValueError(f"opponent index {d} is below the number of learners ({learners}): drone indices "
                             f"0..{learners - 1} are the learners'")
        if d >= N:
            raise ValueError(f"opponent index {d}: the env has drone indices 0..{N - 1}")
        if a is None:
            continue
        if isinstance(a, (str, os.PathLike)):
            a = build_agent(a, params.window_radius, device)
        elif not _is_net(a):
            raise ValueError(f"opponent {d}: a device net (QNetwork / WideQNetwork / ConvQNetwork), a checkpoint "
                             "path or None")
        if a.in_features != W * W * 6 or a.n_actions != 5:
            raise ValueError(f"opponent {d}: a net of {a.in_features} inputs / {a.n_actions} actions cannot drive "
                             f"a {W}x{W} window with 5 actions")
        out[d] = a
    return out


class LeagueLoop:
    """One league step at a time over caller-owned env, league and rings:
    the synthetic columns (if a drone is random), the league act, the fixed
    nets' acts, the env step, every drone's next code, the add, the train."""

    def __init__(self, env, league: LeagueDQN, replay: LeagueReplay, opponents: Optional[Dict[int, object]] = None,
                 action_seed: int = 2024, act_seed: int = 7):
        from .evaluator import obs_code_all
        self.env, self.league, self.replay = env, league, replay
        self.opponents = dict(opponents or {})
        self.action_seed, self.act_seed = action_seed, act_seed
        E, N, dev = env.num_envs, env.n_drones, env.device
        if league.E != E or league.members > N or replay.members != league.members:
            raise ValueError("the league needs one learner per ring, at most one per drone, over the env's batch")
        self.any_random = any(d not in self.opponents for d in range(league.members, N))
        self.codes = [obs_code_all(env), torch.empty((N, E, env.policy_code_bytes), dtype=torch.uint8, device=dev)]
        # (one spare row: a fixed net's act writes column 0 of the [E, N] view that starts at its own column)
        self.flat = torch.zeros(E * N + N, dtype=torch.int32, device=dev)
        self.actions = self.flat[:E * N].view(E, N)
        self.rewards = torch.empty((E, N), dtype=torch.float32, device=dev)
        self.dones = torch.empty((E, N), dtype=torch.uint8, device=dev)
        W = 2 * env.params.window_radius + 1
        self.obs = (torch.empty((E, W * W * 6), dtype=torch.float32, device=dev)
                    if any(a.input != "code" for a in self.opponents.values()) else None)
        self.cur = 0

    def act(self, t: int, greedy: bool = False, q: Optional[torch.Tensor] = None):
        """Every drone's action of step t into self.actions."""
        from .dqn import decode_policy_code
        env, E, N = self.env, self.env.num_envs, self.env.n_drones
        codes = self.codes[self.cur]
        if self.any_random:
            env.synth_actions(self.action_seed, t, out=self.actions)
        self.league.act(codes, t, seed=self.act_seed, env_offset=env.env_offset, actions=self.actions,
                        greedy=greedy, q=q)
        for d, a in self.opponents.items():
            col = self.flat[d:d + E * N].view(E, N)
            rows = codes[d]
            a.act(rows if a.input == "code" else decode_policy_code(rows, env.params.window_radius, out=self.obs),
                  0.0, actions=col)
        return self.actions

    def add(self, nxt: torch.Tensor):
        """The step's transitions (the codes the act read, `nxt` after the
        env step) into the learners' rings."""
        self.replay.add(self.codes[self.cur], self.actions, self.rewards, nxt, self.dones)

    def step(self, t: int, on_step=None, reset: bool = False):
        from .evaluator import obs_code_all
        env = self.env
        self.act(t)
        env.step(self.actions, rewards=self.rewards, dones=self.dones)
        nxt = self.codes[1 - self.cur]
        obs_code_all(env, nxt)
        self.add(nxt)
        if on_step is not None:
            on_step(t, self.league, self.replay, self.actions, self.rewards, self.dones)
        self.league.train(self.replay)
        if reset:
            env.reset(seed=None)
            obs_code_all(env, nxt)
        self.cur = 1 - self.cur


@dataclass
class LeagueResult:
    env: object
    league: LeagueDQN
    replay: LeagueReplay
    steps: int
    agent_steps_per_s: float
    opponents: Dict[int, object] = field(default_factory=dict)


def train_league(params: EnvParams, learners: Sequence[DQNHParams], num_envs: int, num_steps: int,
                 hidden: Sequence[int] = (128, 64), opponents=None, reset_env_every: int = 100,
                 memory_size: int = 100_000, seed: int = 0, env_offset: int = 0, action_seed: int = 2024,
                 act_seed: int = 7, seeds: Optional[Sequence[int]] = None, on_step=None,
                 device=None, network_type: str = "dense", conv_layers=None,
                 conv_dense_layers: Sequence[int] = ()) -> LeagueResult:
    """MultiAgentTrainer.train on the device: per step the synthetic columns,
    the league act (columns 0..K-1), the fixed opponents' greedy acts, one env
    step, every drone's next code, the add into the learners' rings, the
    learners' train blocks, and a reset of every env when
    step % reset_env_every == 0 (train_population's rule).  learners: a
    DQNHParams each; opponents: {drone index >= K: net | checkpoint path |
    None}, missing indices are random; seeds: each learner's initialisation
    seed (default `seed` for all).  on_step(t, league, replay, actions,
    rewards, dones): called between step t's add and its train (tests).
    network_type "conv": every learner a conv net (a ConvLeagueDQN of
    conv_layers, default train_jax.py's one 3x3 layer of 8 channels, padding
    1, and conv_dense_layers; `hidden` is then unused), as train_population
    takes them."""
    from .env import BatchedDeliveryDrones
    if num_steps < 1 or reset_env_every < 1:
        raise ValueError("num_steps and reset_env_every must be >= 1")
    if network_type not in ("dense", "conv"):
        raise ValueError("network_type must be 'dense' or 'conv'")
    learners = list(learners)
    K, E, N = len(learners), int(num_envs), params.n_drones
    if not 1 <= K <= N:
        raise ValueError(f"{K} learners for {N} drones: a league has between 1 learner and one per drone index")
    r = params.window_radius
    env = BatchedDeliveryDrones(params, E, device=device, env_offset=env_offset)
    env.reset(seed=seed)
    dev = env.device
    opp = resolve_opponents(opponents, K, params, dev)
    seeds = seeds if seeds is not None else [seed] * K
    if network_type == "conv":
        from .checkpoint import TRAIN_JAX_CONV_LAYERS
        W = 2 * r + 1
        league = ConvLeagueDQN((W, W, 6), conv_layers if conv_layers is not None else TRAIN_JAX_CONV_LAYERS,
                               tuple(conv_dense_layers), learners, E, device=dev, seeds=seeds)
    else:
        league = LeagueDQN((2 * r + 1) ** 2 * 6, hidden, learners, E, device=dev, seeds=seeds)
    rb = LeagueReplay(K, memory_size, r, device=dev)
    loop = LeagueLoop(env, league, rb, opp, action_seed=action_seed, act_seed=act_seed)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(num_steps):
        loop.step(t, on_step=on_step, reset=t % reset_env_every == 0)
    e1.record()
    torch.cuda.synchronize(dev)
    env.check_errors()
    league.check_errors()
    for a in opp.values():
        a.check_errors()
    dt = e0.elapsed_time(e1) / 1e3
    return LeagueResult(env, league, rb, num_steps, K * num_steps / dt, opp)


def evaluate_league(result_or_nets, params: Optional[EnvParams] = None, opponents=None,
                    seeds: Sequence[int] = (0, 1, 2, 3, 4), num_steps: int = 1000, device=None,
                    action_seed: int = 0) -> dict:
    """The learners, greedy, beside the same opponents in one line-up
    (evaluator.evaluate_lineups): {"scores": float64 [len(seeds), n_drones]
    episode reward sums, "mean", "std": per drone over the episodes,
    "roles"}.  result_or_nets: a LeagueResult (its env parameters and
    opponents are the defaults) or a list of nets / checkpoint paths for
    drone indices 0..K-1."""
    from .evaluator import evaluate_lineups
    if isinstance(result_or_nets, LeagueResult):
        res = result_or_nets
        nets = [res.league.member_net(k, input="code") for k in range(res.league.members)]
        params = params if params is not None else res.env.params
        opponents = opponents if opponents is not None else res.opponents
    else:
        nets = list(result_or_nets)
    if params is None:
        raise ValueError("params: the env the line-up is scored in")
    K, N = len(nets), params.n_drones
    if not 1 <= K <= N:
        raise ValueError(f"{K} learners for {N} drones")
    opp = {int(d): a for d, a in (opponents or {}).items() if a is not None}
    for d in opp:
        if not K <= d < N:
            raise ValueError(f"opponent index {d} must be in [{K}, {N})")
    lineup = nets + [opp.get(d) for d in range(K, N)]
    scores = evaluate_lineups(params, [lineup], list(seeds), num_steps, device=device, action_seed=action_seed)[0]
    roles = [f"learner {k}" for k in range(K)] + ["opponent" if d in opp else "random" for d in range(K, N)]
    return {"scores": scores, "mean": scores.mean(axis=0), "std": scores.std(axis=0), "roles": roles}


# ------------------------------------------------------------ command line --
CONV_LEARNERS_REFUSAL = ("--network_type conv: a league's learners are dense nets (conv learners train with "
                         "python -m dronerl_amd.conv_league; conv checkpoints work as --opponents)")
SHARDING_REFUSAL = "a league runs on one GPU (no --use_sharding): sharded leagues are not implemented"


def opponents_of(items: Sequence[str], learners: int, n_drones: int) -> Dict[int, Optional[str]]:
    """--opponents' words as {drone index: path or None}.  A word is PATH
    (the next drone index from K upwards that no word names), INDEX=PATH, or
    `random` in PATH's place."""
    named, plain = {}, []
    for w in items:
        head, sep, tail = w.partition("=")
        if sep and head.lstrip("-").isdigit():
            d = int(head)
            if d < learners:
                raise ValueError(f"--opponents {w}: opponent index {d} is below the number of learners "
                                 f"({learners}); drone indices 0..{learners - 1} are the learners'")
            if d >= n_drones:
                raise ValueError(f"--opponents {w}: the env has drone indices 0..{n_drones - 1}")
            if d in named:
                raise ValueError(f"--opponents: drone index {d} is named twice")
            named[d] = tail
        else:
            plain.append(w)
    free = [d for d in range(learners, n_drones) if d not in named]
    if len(plain) > len(free):
        raise ValueError(f"--opponents: {len(plain) + len(named)} opponents and {learners} learners do not fit "
                         f"{n_drones} drones")
    named.update(zip(free, plain))
    return {d: (None if p.lower() == "random" else p) for d, p in sorted(named.items())}


def parse_args(argv=None):
    """train.parse_args plus --learners, --opponents and --grid.  Returns
    (args, points): the shared options (args.learners, args.opponents: the
    drone-index map) and the grid's points, one per learner or one shared."""
    import argparse

    from .sweep import expand_grid
    from .train import parse_args as train_args
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--learners", type=int, default=2)
    ap.add_argument("--opponents", nargs="*", default=[])
    ap.add_argument("--grid", type=str, default="{}")
    own, rest = ap.parse_known_args(argv)
    args = train_args(rest)
    from .train import refuse_prioritized
    refuse_prioritized(args, "the league")
    if args.network_type != "dense":
        raise ValueError(CONV_LEARNERS_REFUSAL)
    if args.use_sharding:
        raise ValueError(SHARDING_REFUSAL)
    if own.learners < 1:
        raise ValueError("--learners must be >= 1")
    if own.learners > args.n_drones:
        raise ValueError(f"--learners {own.learners}: more learners than drones (--n_drones {args.n_drones}); "
                         "learner k drives drone index k")
    try:
        grid = json.loads(own.grid)
    except json.JSONDecodeError as e:
        raise ValueError(f"--grid is not valid JSON: {e}")
    points = expand_grid(grid)
    from .train import refuse_double_dqn
    refuse_double_dqn(args, "the league", points)
    if len(points) not in (1, own.learners):
        raise ValueError(f"--grid has {len(points)} points: one per learner ({own.learners}) or one shared point")
    args.learners = own.learners
    args.opponents = opponents_of(own.opponents, own.learners, args.n_drones)
    return args, points


def learners_of(args, points) -> List[DQNHParams]:
    """A DQNHParams per learner: learner k takes grid point k (or the one
    shared point) over the shared options; its replay draw is seeded
    seed + k."""
    import copy

    from .train import hparams_of
    hps = []
    for k in range(args.learners):
        a = copy.copy(args)
        for key, v in points[k if len(points) > 1 else 0].items():
            setattr(a, key, type(getattr(args, key))(v) if getattr(args, key) is not None else v)
        a.seed = args.seed + k
        hps.append(hparams_of(a))
    return hps


def main(argv=None) -> dict:
    """Train the league, save every learner, score the greedy line-up."""
    from datetime import datetime

    from .train import env_params_of
    args, points = parse_args(argv)
    hps = learners_of(args, points)
    dev = torch.device("cuda", torch.cuda.current_device())
    K = args.learners
    res = train_league(env_params_of(args), hps, args.num_envs, args.num_steps, hidden=tuple(args.hidden_layers),
                       opponents=args.opponents, reset_env_every=args.reset_env_every,
                       memory_size=args.memory_size, seed=args.seed, seeds=[args.seed + k for k in range(K)],
                       device=dev)
    out = {"learners": K, "num_envs": args.num_envs, "num_steps": args.num_steps,
           "hidden_layers": list(args.hidden_layers), "steps_per_sec": res.agent_steps_per_s / K,
           "agent_steps_per_sec": res.agent_steps_per_s,
           "opponents": {str(d): p for d, p in args.opponents.items()}}
    if args.save_final_checkpoint:
        run_dir = os.path.join(args.output_dir, f"league_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
        os.makedirs(run_dir, exist_ok=True)
        out["checkpoints"] = []
        for k in range(K):
            paths = {}
            for fmt in ("jax", "torch"):
                paths[fmt] = os.path.join(run_dir, f"learner_{k}_agent_{args.num_steps}_steps_{fmt}.safetensors")
                res.league.save(k, paths[fmt], format=fmt)
            out["checkpoints"].append(paths)
    ev = evaluate_league(res, params=env_params_of(args, eval_env=True),
                         seeds=[args.eval_seed + i for i in range(args.num_evals)], num_steps=args.num_eval_steps,
                         device=dev, action_seed=args.eval_seed)
    out["eval"] = [{"drone": d, "role": ev["roles"][d], "reward_mean": float(ev["mean"][d]),
                    "reward_std": float(ev["std"][d]),
                    **({"final_epsilon": res.league.counters(d)["epsilon"],
                        "train_steps": res.league.counters(d)["count"]} if d < K else {})}
                   for d in range(len(ev["roles"]))]
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
