"""Shared-policy self-play: a Q-network trained on several drones of every
env (include/dronerl.h drl_selfplay_*; dronerl_amd/csrc/selfplay/ for dense
learners, drl_convselfplay_act and dronerl_amd/csrc/convselfplay/ for conv
learners).

Reference: torch_impl/helpers/rl_helpers.py:44-65, MultiAgentTrainer.train
walks its `agents` dict; an agent object that sits under several keys acts
for every one of those drones and remembers every one of their transitions
in its one memory.

One batch of E envs with N drones each and K learners, each driving a TEAM
of M drone indices, K * M <= N: `drones[k][j]` (default k * M + j) is the
j-th drone of learner k.  Each learner is exactly a population member, as in
the league (`LeagueDQN`): `train`, the block and the rings are the
population's, unchanged.  Ring k takes the M * E transitions of its team per
env step in the order (team slot j, env i) -- ReplayBuffer.add_many on those
rows -- so the one cursor advances by M * E.  Drones in no team are random or
fixed nets, exactly as in the league.

The exploration draw of drone dr in env i is
explore_draw(seed + dr, step, env_offset + i, n_actions, epsilon_k): keyed on
the drone index, so two drones of a team never share a stream and a team of
one on drone k is the league's learner k, bit for bit.

One learner step per env step (train_jax.py's block: add all rows, then one
train_step); the reference's per-key `learn` calls would make M.

    train_selfplay(params, learners, drones_per_learner, num_envs, num_steps) -> SelfPlayResult
    evaluate_selfplay(result)                                    -> the greedy table
    python -m dronerl_amd.selfplay --learners 1 --drones_per_learner 4 --n_drones 6 ...

Conv learners (`ConvSelfPlayDQN`, train_selfplay(network_type="conv")) have
their own command line, `python -m dronerl_amd.conv_selfplay`.
"""
from __future__ import annotations

import ctypes
import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Union

import torch

from .dqn import DQNHParams, DrlReplay, DrlWidenetDesc, _check, _on, _stream, _vp
from .league import U64, ConvLeagueDQN, LeagueDQN, LeagueLoop, _bind_convleague, _bind_league, resolve_opponents
from .params import EnvParams
from .population import PopulationReplay


def _bind_selfplay(L):
    if getattr(L, "_selfplay_ready", False):
        return L
    _bind_league(L)
    i32, i64, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    D, R = ctypes.POINTER(DrlWidenetDesc), ctypes.POINTER(DrlReplay)
    sig = {
        "drl_selfplay_act": [D, i32, i32, _vp, _vp, i64, _vp, i32, i32, u64, u64, i64, _vp, i32, _vp, _vp],
        "drl_selfplay_replay_add": [D, i32, R, i64, i64, _vp, i32, _vp, _vp, _vp, _vp, _vp, i32, _vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = ctypes.c_int
    L._selfplay_ready = True
    return L


def _bind_convselfplay(L):
    if getattr(L, "_convselfplay_ready", False):
        return L
    from .dqn import DrlConvnetDesc
    _bind_convleague(L)
    i32, i64, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    D = ctypes.POINTER(DrlConvnetDesc)
    f = L.drl_convselfplay_act
    f.argtypes = [D, i32, i32, _vp, _vp, i64, _vp, i32, i32, u64, u64, i64, _vp, i32, _vp, _vp]
    f.restype = ctypes.c_int
    L._convselfplay_ready = True
    return L


def default_drones(learners: int, team: int) -> List[List[int]]:
    """drones[k][j] = k * team + j."""
    return [[k * team + j for j in range(team)] for k in range(learners)]


def team_map(drones) -> List[List[int]]:
    """`drones` as K lists of the same M >= 1 ints (the library checks the
    indices themselves against n_drones)."""
    out = [[int(d) for d in row] for row in drones]
    if not out or not out[0] or any(len(row) != len(out[0]) for row in out):
        raise ValueError("drones: one list per learner, all of the same length >= 1 (every learner drives the same "
                         "number of drones: the rings share one cursor)")
    return out


def _c_map(drones: List[List[int]]):
    flat = [d for row in drones for d in row]
    return (ctypes.c_int32 * len(flat))(*flat)


class SelfPlayReplay(PopulationReplay):
    """K replay rings in one allocation, ring k fed by the M drones of
    learner k's team (drl_selfplay_replay_add): drone drones[k][j] of env i
    lands in slot (cursor + j * E + i) % capacity, and an add larger than the
    ring keeps its last `capacity` rows.  The layout, cursor and size are
    PopulationReplay's."""

    def __init__(self, members: int, capacity: int, window_radius: int, device=None):
        super().__init__(members, capacity, window_radius, device=device)
        _bind_selfplay(self.L)

    def add(self, codes_prev: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, codes: torch.Tensor,
            dones: torch.Tensor, drones):
        """codes_prev / codes: uint8 [n_drones, E, code_bytes]
        (evaluator.obs_code_all: what the act read, what the step left);
        actions i32, rewards f32, dones u8 [E, n_drones]; drones: K lists of
        M drone indices.  Advances cursor and size by M * E."""
        dev = self.obs.device
        drones = team_map(drones)
        if len(drones) != self.members:
            raise ValueError(f"drones: {len(drones)} teams for {self.members} rings")
        for t, dt, name in ((codes_prev, torch.uint8, "codes_prev"), (codes, torch.uint8, "codes"),
                            (actions, torch.int32, "actions"), (rewards, torch.float32, "rewards"),
                            (dones, torch.uint8, "dones")):
            _on(t, dev, dt, name)
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        if codes.dim() != 3 or codes.shape != codes_prev.shape or codes.shape[2] != self.code_bytes:
            raise ValueError(f"codes and codes_prev must be uint8 [n_drones, E, {self.code_bytes}]")
        N, E, M = int(codes.shape[0]), int(codes.shape[1]), len(drones[0])
        for t, name in ((actions, "actions"), (rewards, "rewards"), (dones, "dones")):
            if tuple(t.shape) != (E, N):
                raise ValueError(f"{name} must be [{E}, {N}] (envs by drones)")
        _check(self.L, self.L.drl_selfplay_replay_add(
            ctypes.byref(self.desc), self.members, ctypes.byref(self._c), self.cursor, E, _c_map(drones), M,
            _vp(codes_prev.data_ptr()), _vp(codes.data_ptr()), _vp(actions.data_ptr()), _vp(rewards.data_ptr()),
            _vp(dones.data_ptr()), N, _stream(dev)))
        self.cursor = (self.cursor + M * E) % self.capacity
        self.size = min(self.size + M * E, self.capacity)


DOUBLE_SELFPLAY_REFUSAL = ("double_dqn: self-play learners (SelfPlayDQN, ConvSelfPlayDQN) train the max rule only; "
                           "Double DQN is implemented for single dense agents and dense populations")


class SelfPlayDQN(LeagueDQN):
    """K learners over the same E envs, learner k on the drones
    `drones[k]` (K lists of M distinct drone indices; default k * M + j with
    M = `team`): a PopulationDQN with members = K whose act runs learner k's
    weights on the code rows of each of its drones and writes those drones'
    columns of the action matrix (drl_selfplay_act).  `train`, `member_net`,
    `save`, `params`, `counters` and `sample_slots` are the population's."""

    _double_refusal = DOUBLE_SELFPLAY_REFUSAL

    def __init__(self, in_features: int, hidden: Sequence[int], hps: Sequence[DQNHParams], num_envs: int,
                 drones=None, team: int = 1, **kw):
        super().__init__(in_features, hidden, hps, num_envs, **kw)
        _bind_selfplay(self.L)
        self.drones = team_map(drones) if drones is not None else default_drones(self.members, int(team))
        if len(self.drones) != self.members:
            raise ValueError(f"drones: {len(self.drones)} teams for {self.members} learners")
        self.team = len(self.drones[0])
        self._map = _c_map(self.drones)

    def act(self, codes: torch.Tensor, step: int, seed: int = 0, env_offset: int = 0,
            actions: Optional[torch.Tensor] = None, greedy: bool = False,
            q: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The teams' columns of actions [E, n_drones] (no other column is
        written): for dr = drones[k][j], learner k's epsilon-greedy action of
        env i from its online net on codes[dr, i] and its device epsilon
        (greedy: no exploration), the draw keyed on (seed + dr, step,
        env_offset + i).  codes: uint8 [n_drones, E, code_bytes]
        (evaluator.obs_code_all).  q: float32 [K, M, E, n_actions]."""
        K, M, E = self.members, self.team, self.E
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
            if tuple(q.shape) != (K, M, E, self.n_actions) or not q.is_contiguous():
                raise ValueError(f"q must be a contiguous float32 [{K}, {M}, {E}, {self.n_actions}] tensor")
        _check(self.L, self.L.drl_selfplay_act(
            ctypes.byref(self.desc), K, self.max_batch, _vp(self.block.data_ptr()), _vp(codes.data_ptr()), E,
            self._map, M, int(bool(greedy)), int(seed) & U64, int(step), int(env_offset), _vp(actions.data_ptr()), N,
            None if q is None else _vp(q.data_ptr()), _stream(self.device)))
        return actions


class ConvSelfPlayDQN(ConvLeagueDQN):
    """SelfPlayDQN for conv learners: K conv learners over the same E envs,
    learner k on the drones `drones[k]` (K lists of M distinct drone indices;
    default k * M + j with M = `team`): a ConvPopulationDQN with members = K
    whose act runs learner k's forward on the code rows of each of its drones
    and writes those drones' columns of the action matrix
    (drl_convselfplay_act: the conv league act's tiling on the learner's
    M * E rows; Q is drl_convpop_act's bit for bit).  `train`, `member_net`,
    `save`, `params`, `counters` and `sample_slots` are the conv
    population's."""

    _double_refusal = DOUBLE_SELFPLAY_REFUSAL

    def __init__(self, obs_shape, conv_layers, dense_layers: Sequence[int], hps: Sequence[DQNHParams],
                 num_envs: int, drones=None, team: int = 1, **kw):
        super().__init__(obs_shape, conv_layers, dense_layers, hps, num_envs, **kw)
        _bind_convselfplay(self.L)
        self.drones = team_map(drones) if drones is not None else default_drones(self.members, int(team))
        if len(self.drones) != self.members:
            raise ValueError(f"drones: {len(self.drones)} teams for {self.members} learners")
        self.team = len(self.drones[0])
        self._map = _c_map(self.drones)

    def act(self, codes: torch.Tensor, step: int, seed: int = 0, env_offset: int = 0,
            actions: Optional[torch.Tensor] = None, greedy: bool = False,
            q: Optional[torch.Tensor] = None) -> torch.Tensor:
        """SelfPlayDQN.act's arguments, checks and result (q: float32
        [K, M, E, n_actions])."""
        K, M, E = self.members, self.team, self.E
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
            if tuple(q.shape) != (K, M, E, self.n_actions) or not q.is_contiguous():
                raise ValueError(f"q must be a contiguous float32 [{K}, {M}, {E}, {self.n_actions}] tensor")
        _check(self.L, self.L.drl_convselfplay_act(
            ctypes.byref(self.desc), K, self.max_batch, _vp(self.block.data_ptr()), _vp(codes.data_ptr()), E,
            self._map, M, int(bool(greedy)), int(seed) & U64, int(step), int(env_offset), _vp(actions.data_ptr()), N,
            None if q is None else _vp(q.data_ptr()), _stream(self.device)))
        return actions


def resolve_team_opponents(opponents, drones, params: EnvParams, device=None) -> Dict[int, object]:
    """league.resolve_opponents for drone indices that no team holds."""
    held = {d: k for k, row in enumerate(drones) for d in row}
    for d in (opponents or {}):
        if int(d) in held:
            raise ValueError(f"opponent index {int(d)} is inside learner {held[int(d)]}'s team: an opponent takes a "
                             "drone index that no team holds")
    return resolve_opponents(opponents, 0, params, device)


class SelfPlayLoop(LeagueLoop):
    """LeagueLoop's step, in its order, for learners that drive teams: the
    synthetic columns (if a drone is random), the self-play act, the fixed
    nets' acts, the env step, every drone's next code, the add of every
    team's rows, the train."""

    def __init__(self, env, league: Union[SelfPlayDQN, ConvSelfPlayDQN], replay: SelfPlayReplay,
                 opponents: Optional[Dict[int, object]] = None, action_seed: int = 2024, act_seed: int = 7):
        super().__init__(env, league, replay, opponents, action_seed=action_seed, act_seed=act_seed)
        held = {d for row in league.drones for d in row}
        if len(held) > env.n_drones or any(d in held for d in self.opponents):
            raise ValueError("a drone index has one driver: at most n_drones team drones, no opponent inside a team")
        self.any_random = any(d not in held and d not in self.opponents for d in range(env.n_drones))

    def add(self, nxt: torch.Tensor):
        self.replay.add(self.codes[self.cur], self.actions, self.rewards, nxt, self.dones, self.league.drones)


@dataclass
class SelfPlayResult:
    env: object
    league: Union[SelfPlayDQN, ConvSelfPlayDQN]
    replay: SelfPlayReplay
    steps: int
    agent_steps_per_s: float   # learner steps (one per learner and env step) per second
    rows_per_s: float          # transitions landed in the rings per second (K * M * E per env step)
    opponents: Dict[int, object] = field(default_factory=dict)


def train_selfplay(params: EnvParams, learners: Sequence[DQNHParams], drones_per_learner: int, num_envs: int,
                   num_steps: int, hidden: Sequence[int] = (128, 64), drones=None, opponents=None,
                   reset_env_every: int = 100, memory_size: int = 100_000, seed: int = 0, env_offset: int = 0,
                   action_seed: int = 2024, act_seed: int = 7, seeds: Optional[Sequence[int]] = None, on_step=None,
                   device=None, network_type: str = "dense", conv_layers=None,
                   conv_dense_layers: Sequence[int] = ()) -> SelfPlayResult:
    """train_league with every learner on `drones_per_learner` drones: per
    step the synthetic columns, the self-play act (the teams' columns), the
    fixed opponents' greedy acts, one env step, every drone's next code, the
    add of every team's M * E rows into its learner's ring, ONE train block
    per learner, and a reset of every env when step % reset_env_every == 0.
    learners: a DQNHParams each; drones: K lists of M drone indices (default
    k * M + j); opponents: {drone index in no team: net | checkpoint path |
    None}, missing indices are random; seeds: each learner's initialisation
    seed (default `seed` for all).  on_step(t, league, replay, actions,
    rewards, dones): called between step t's add and its train (tests).
    network_type "conv": every learner a conv net (a ConvSelfPlayDQN of
    conv_layers, default train_jax.py's one 3x3 layer of 8 channels, padding
    1, and conv_dense_layers; `hidden` is then unused), as train_league takes
    them."""
    from .env import BatchedDeliveryDrones
    if num_steps < 1 or reset_env_every < 1:
        raise ValueError("num_steps and reset_env_every must be >= 1")
    if network_type not in ("dense", "conv"):
        raise ValueError("network_type must be 'dense' or 'conv'")
    learners = list(learners)
    K, M, E, N = len(learners), int(drones_per_learner), int(num_envs), params.n_drones
    if K < 1 or M < 1 or K * M > N:
        raise ValueError(f"{K} learners of {M} drones each for {N} drones: K * M must be in [1, n_drones]")
    drones = team_map(drones) if drones is not None else default_drones(K, M)
    if len(drones) != K or len(drones[0]) != M:
        raise ValueError(f"drones must be {K} lists of {M} drone indices")
    r = params.window_radius
    env = BatchedDeliveryDrones(params, E, device=device, env_offset=env_offset)
    env.reset(seed=seed)
    dev = env.device
    opp = resolve_team_opponents(opponents, drones, params, dev)
    seeds = seeds if seeds is not None else [seed] * K
    if network_type == "conv":
        from .checkpoint import TRAIN_JAX_CONV_LAYERS
        W = 2 * r + 1
        league = ConvSelfPlayDQN((W, W, 6), conv_layers if conv_layers is not None else TRAIN_JAX_CONV_LAYERS,
                                 tuple(conv_dense_layers), learners, E, drones=drones, device=dev, seeds=seeds)
    else:
        league = SelfPlayDQN((2 * r + 1) ** 2 * 6, hidden, learners, E, drones=drones, device=dev, seeds=seeds)
    rb = SelfPlayReplay(K, memory_size, r, device=dev)
    loop = SelfPlayLoop(env, league, rb, opp, action_seed=action_seed, act_seed=act_seed)
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
    return SelfPlayResult(env, league, rb, num_steps, K * num_steps / dt, K * M * E * num_steps / dt, opp)


def evaluate_selfplay(result_or_nets, params: Optional[EnvParams] = None, drones=None, opponents=None,
                      seeds: Sequence[int] = (0, 1, 2, 3, 4), num_steps: int = 1000, device=None,
                      action_seed: int = 0) -> dict:
    """The learners, greedy, each on every drone of its team, beside the same
    opponents in one line-up (evaluator.evaluate_lineups); evaluate_league's
    dict: {"scores": float64 [len(seeds), n_drones] episode reward sums,
    "mean", "std": per drone over the episodes, "roles"}.  result_or_nets: a
    SelfPlayResult (its env parameters, teams and opponents are the defaults)
    or a list of K nets / checkpoint paths with `drones` (K lists)."""
    from .evaluator import evaluate_lineups
    if isinstance(result_or_nets, SelfPlayResult):
        res = result_or_nets
        nets = [res.league.member_net(k, input="code") for k in range(res.league.members)]
        params = params if params is not None else res.env.params
        drones = drones if drones is not None else res.league.drones
        opponents = opponents if opponents is not None else res.opponents
    else:
        nets = list(result_or_nets)
    if params is None or drones is None:
        raise ValueError("params: the env the line-up is scored in; drones: each net's drone indices")
    drones, N = team_map(drones), params.n_drones
    held = {d: k for k, row in enumerate(drones) for d in row}
    if len(drones) != len(nets) or len(held) != len(nets) * len(drones[0]) or not all(0 <= d < N for d in held):
        raise ValueError(f"drones: one team of distinct drone indices in [0, {N}) per net")
    opp = {int(d): a for d, a in (opponents or {}).items() if a is not None}
    for d in opp:
        if d in held or not 0 <= d < N:
            raise ValueError(f"opponent index {d} must be a drone index in [0, {N}) that no team holds")
    lineup = [nets[held[d]] if d in held else opp.get(d) for d in range(N)]
    scores = evaluate_lineups(params, [lineup], list(seeds), num_steps, device=device, action_seed=action_seed)[0]
    roles = [f"learner {held[d]}" if d in held else "opponent" if d in opp else "random" for d in range(N)]
    return {"scores": scores, "mean": scores.mean(axis=0), "std": scores.std(axis=0), "roles": roles}


# ------------------------------------------------------------ command line --
CONV_LEARNERS_REFUSAL = ("--network_type conv: this command's self-play learners are dense nets (conv learners train one "
                         "drone each with python -m dronerl_amd.conv_league and several with python -m "
                         "dronerl_amd.conv_selfplay; conv checkpoints work as --opponents)")
SHARDING_REFUSAL = ("self-play runs on one GPU (no --use_sharding): python -m dronerl_amd.train --use_sharding shards "
                    "one learner on drone 0")


def drones_of(word: Optional[str], learners: int, team: int, n_drones: int) -> List[List[int]]:
    """--drones' comma-separated K * M drone indices as the [K][M] map
    (learner k takes words k * M .. k * M + M - 1); None: the default map."""
    if learners < 1 or team < 1:
        raise ValueError("--learners and --drones_per_learner must be >= 1")
    if learners * team > n_drones:
        raise ValueError(f"--learners {learners} x --drones_per_learner {team}: more team drones than drones "
                         f"(--n_drones {n_drones}); a drone index has at most one learner")
    if word is None:
        return default_drones(learners, team)
    try:
        flat = [int(w) for w in word.split(",")]
    except ValueError:
        raise ValueError(f"--drones {word}: comma-separated drone indices")
    if len(flat) != learners * team:
        raise ValueError(f"--drones names {len(flat)} drone indices: {learners} learners x {team} drones each need "
                         f"{learners * team}")
    if len(set(flat)) != len(flat):
        raise ValueError(f"--drones {word}: a drone index is named twice")
    if not all(0 <= d < n_drones for d in flat):
        raise ValueError(f"--drones {word}: the env has drone indices 0..{n_drones - 1}")
    return [flat[k * team:(k + 1) * team] for k in range(learners)]


def opponents_of(items: Sequence[str], drones: List[List[int]], n_drones: int) -> Dict[int, Optional[str]]:
    """--opponents' words as {drone index: path or None}.  A word is PATH
    (the next drone index, upwards, that no team holds and no word names),
    INDEX=PATH, or `random` in PATH's place."""
    held = {d: k for k, row in enumerate(drones) for d in row}
    named, plain = {}, []
    for w in items:
        head, sep, tail = w.partition("=")
        if sep and head.lstrip("-").isdigit():
            d = int(head)
            if d in held:
                raise ValueError(f"--opponents {w}: opponent index {d} is inside learner {held[d]}'s team; an "
                                 "opponent takes a drone index that no team holds")
            if not 0 <= d < n_drones:
                raise ValueError(f"--opponents {w}: the env has drone indices 0..{n_drones - 1}")
            if d in named:
                raise ValueError(f"--opponents: drone index {d} is named twice")
            named[d] = tail
        else:
            plain.append(w)
    free = [d for d in range(n_drones) if d not in held and d not in named]
    if len(plain) > len(free):
        raise ValueError(f"--opponents: {len(plain) + len(named)} opponents and {len(held)} team drones do not fit "
                         f"{n_drones} drones")
    named.update(zip(free, plain))
    return {d: (None if p.lower() == "random" else p) for d, p in sorted(named.items())}


def parse_args(argv=None):
    """train.parse_args plus --learners, --drones_per_learner, --drones,
    --opponents and --grid.  Returns (args, points): the shared options
    (args.learners, args.drones_per_learner, args.drones: the [K][M] map,
    args.opponents: the drone-index map) and the grid's points, one per
    learner or one shared."""
    import argparse

    from .sweep import expand_grid
    from .train import parse_args as train_args
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--learners", type=int, default=1)
    ap.add_argument("--drones_per_learner", type=int, default=2)
    ap.add_argument("--drones", type=str, default=None)
    ap.add_argument("--opponents", nargs="*", default=[])
    ap.add_argument("--grid", type=str, default="{}")
    own, rest = ap.parse_known_args(argv)
    args = train_args(rest)
    from .train import refuse_prioritized
    refuse_prioritized(args, "self-play")
    if args.network_type != "dense":
        raise ValueError(CONV_LEARNERS_REFUSAL)
    if args.use_sharding:
        raise ValueError(SHARDING_REFUSAL)
    drones = drones_of(own.drones, own.learners, own.drones_per_learner, args.n_drones)
    try:
        grid = json.loads(own.grid)
    except json.JSONDecodeError as e:
        raise ValueError(f"--grid is not valid JSON: {e}")
    points = expand_grid(grid)
    from .train import refuse_double_dqn
    refuse_double_dqn(args, "self-play", points)
    if len(points) not in (1, own.learners):
        raise ValueError(f"--grid has {len(points)} points: one per learner ({own.learners}) or one shared point")
    args.learners, args.drones_per_learner, args.drones = own.learners, own.drones_per_learner, drones
    args.opponents = opponents_of(own.opponents, drones, args.n_drones)
    return args, points


def main(argv=None) -> dict:
    """Train the learners on their teams, save every learner, score the
    greedy line-up."""
    from datetime import datetime

    from .league import learners_of
    from .train import env_params_of
    args, points = parse_args(argv)
    hps = learners_of(args, points)
    dev = torch.device("cuda", torch.cuda.current_device())
    K, M = args.learners, args.drones_per_learner
    res = train_selfplay(env_params_of(args), hps, M, args.num_envs, args.num_steps,
                         hidden=tuple(args.hidden_layers), drones=args.drones, opponents=args.opponents,
                         reset_env_every=args.reset_env_every, memory_size=args.memory_size, seed=args.seed,
                         seeds=[args.seed + k for k in range(K)], device=dev)
    out = {"learners": K, "drones_per_learner": M, "drones": args.drones, "num_envs": args.num_envs,
           "num_steps": args.num_steps, "hidden_layers": list(args.hidden_layers),
           "steps_per_sec": res.agent_steps_per_s / K, "agent_steps_per_sec": res.agent_steps_per_s,
           "replay_rows_per_sec": res.rows_per_s, "opponents": {str(d): p for d, p in args.opponents.items()}}
    if args.save_final_checkpoint:
        run_dir = os.path.join(args.output_dir, f"selfplay_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
        os.makedirs(run_dir, exist_ok=True)
        out["checkpoints"] = []
        for k in range(K):
            paths = {}
            for fmt in ("jax", "torch"):
                paths[fmt] = os.path.join(run_dir, f"learner_{k}_agent_{args.num_steps}_steps_{fmt}.safetensors")
                res.league.save(k, paths[fmt], format=fmt)
            out["checkpoints"].append(paths)
    ev = evaluate_selfplay(res, params=env_params_of(args, eval_env=True),
                           seeds=[args.eval_seed + i for i in range(args.num_evals)], num_steps=args.num_eval_steps,
                           device=dev, action_seed=args.eval_seed)
    held = {d: k for k, row in enumerate(args.drones) for d in row}
    out["eval"] = [{"drone": d, "role": ev["roles"][d], "reward_mean": float(ev["mean"][d]),
                    "reward_std": float(ev["std"][d]),
                    **({"final_epsilon": res.league.counters(held[d])["epsilon"],
                        "train_steps": res.league.counters(held[d])["count"]} if d in held else {})}
                   for d in range(len(ev["roles"]))]
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
