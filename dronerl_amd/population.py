"""A population of DQN agents trained side by side on one GPU: dense nets
(include/dronerl.h drl_pop_*; dronerl_amd/csrc/population/) or conv nets
(drl_convpop_*; dronerl_amd/csrc/convpop/; ConvPopulationDQN).

Reference: run_jax_sweep.py (1,000 train_jax.py runs that differ in
num_envs, batch_size, learning_rate, epsilon_end and the net) and
torch_impl/sweep.py (gamma, decay, target interval, batch).  There, and with
`dronerl_amd.train`, the runs go one after another, each launch-bound.  Here
P agents ("members") -- each exactly train_jax.py:38-115's learner block on
its own envs, with its own weights, hyperparameters and replay ring -- act
and learn in the same launches: one step of the whole population is one
chain of launches whose length does not depend on P.

One BatchedDeliveryDrones of P * E envs serves the population; member m owns
envs m*E .. m*E + E - 1.  Env seeding, the synthetic actions of drones
1..N-1 and drone 0's exploration draw are keyed on the global env index, so
member m is reproduced, bit for bit, by a population of one with
env_offset = m*E.  The population's act is an f32 forward in the learner's
own summation order (its Q equals oracle/dqn_learner.py's `forward` bit for
bit); QNetwork's and WideQNetwork's MFMA acts agree with it to ~1e-5, so a
member reproduces under this API, not necessarily under `train()`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from ._native import DroneRLError, lib
from .dqn import (INPUTS, NUM_ACTIONS, ConvQNetwork, DQNHParams, DrlConvnetDesc, DrlConvnetDqnLayout, DrlDqnHParams,
                  DrlDqnLayout, DrlPerHParams, DrlPerLayout, DrlReplay, DrlWidenetDesc, QNetwork, WideQNetwork, _bind, _bind_convnet, _check, _on,
                  _stream, _vp, convnet_desc, flax_kernel_init, is_wide)
from .params import EnvParams

POP_MAX_MEMBERS = 1024  # DRL_POP_MAX_MEMBERS
SETS = ("online", "target", "m", "v")


class DrlPopLayout(ctypes.Structure):
    _fields_ = [("member", DrlDqnLayout), ("member_stride", ctypes.c_int64), ("hparams_off", ctypes.c_int64),
                ("hparams_stride", ctypes.c_int64), ("bytes", ctypes.c_int64), ("members", ctypes.c_int32),
                ("max_batch", ctypes.c_int32)]


def _bind_pop(L):
    if getattr(L, "_pop_ready", False):
        return L
    i32, i64, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    D, R = ctypes.POINTER(DrlWidenetDesc), ctypes.POINTER(DrlReplay)
    sig = {
        "drl_pop_layout_query": [D, i32, i32, ctypes.POINTER(DrlPopLayout)],
        "drl_pop_init": [D, i32, i32, ctypes.POINTER(DrlDqnHParams), ctypes.POINTER(ctypes.c_float), _vp, _vp],
        "drl_pop_act": [D, i32, i32, _vp, _vp, i64, i32, u64, u64, i64, _vp, i32, u64, u64, _vp, _vp],
        "drl_pop_replay_add": [D, i32, R, i64, i64, _vp, _vp, _vp, _vp, _vp, i32, _vp],
        "drl_pop_train": [D, i32, i32, _vp, R, i64, _vp],
        "drl_pop_sample_rows": [D, i32, i32, _vp, i64, _vp, _vp],
        "drl_pop_double_train": [D, i32, i32, _vp, R, i64, _vp, _vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = ctypes.c_int
    L._pop_ready = True
    return L


def pop_desc(in_features: int, hidden: Sequence[int], n_actions: int = NUM_ACTIONS) -> DrlWidenetDesc:
    """The shared architecture: a dense net on the policy code."""
    hidden = tuple(int(w) for w in hidden)
    if not 1 <= len(hidden) <= 3:
        raise ValueError("hidden: 1 to 3 widths (n_hidden)")
    return DrlWidenetDesc(int(in_features), len(hidden), (ctypes.c_int32 * 3)(*hidden, *[0] * (3 - len(hidden))),
                          int(n_actions), INPUTS["code"])


class PopulationReplay:
    """P replay rings in one allocation (jax_impl/buffers.py ReplayBuffer per
    member; policy-code rows): ring m holds rows m*capacity .. of the five
    arrays.  `add` is ReplayBuffer.add_many for every member at once
    (drl_pop_replay_add): env m*E + i lands in slot (cursor + i) % capacity of
    ring m, and an add larger than the ring keeps its last `capacity` rows.
    The cursor and the size are equal for every member and live here."""

    def __init__(self, members: int, capacity: int, window_radius: int, device=None):
        self.L = _bind_pop(_bind(lib()))
        self.members, self.capacity, self.code_radius = int(members), int(capacity), int(window_radius)
        if self.members < 1 or self.capacity < 1:
            raise ValueError("members and capacity must be >= 1")
        self.code_bytes = int(self.L.drl_policy_code_bytes(self.code_radius))
        if self.code_bytes <= 0:
            raise ValueError("bad window_radius")
        W = 2 * self.code_radius + 1
        self.desc = pop_desc(W * W * 6, (8,))  # (the add reads the window of it alone)
        d = torch.device(device if device is not None else "cuda")
        n = self.members * self.capacity
        self.obs = torch.zeros((n, self.code_bytes), dtype=torch.uint8, device=d)
        self.next_obs = torch.zeros((n, self.code_bytes), dtype=torch.uint8, device=d)
        self.actions = torch.zeros(n, dtype=torch.int32, device=d)
        self.rewards = torch.zeros(n, dtype=torch.float32, device=d)
        self.dones = torch.zeros(n, dtype=torch.uint8, device=d)
        self.cursor = 0
        self.size = 0
        self._c = DrlReplay(self.capacity, self.code_bytes // 4, self.obs.data_ptr(), self.next_obs.data_ptr(),
                            self.actions.data_ptr(), self.rewards.data_ptr(), self.dones.data_ptr())

    def add(self, code_prev: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, code: torch.Tensor,
            dones: torch.Tensor):
        """code_prev / code: uint8 [P*E, code_bytes] (the rows the act read,
        the rows the step wrote); actions i32, rewards f32, dones u8
        [P*E, n_drones] (column 0 taken)."""
        dev = self.obs.device
        n = code.shape[0]
        if n % self.members:
            raise ValueError("the env batch must hold the same number of envs for every member")
        for t, dt, name in ((code_prev, torch.uint8, "code_prev"), (code, torch.uint8, "code"),
                            (actions, torch.int32, "actions"), (rewards, torch.float32, "rewards"),
                            (dones, torch.uint8, "dones")):
            _on(t, dev, dt, name)
            if t.dim() != 2 or t.shape[0] != n or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous [{n}, ...] tensor")
        if code.shape[1] != self.code_bytes or code_prev.shape[1] != self.code_bytes:
            raise ValueError(f"code rows must hold code_bytes={self.code_bytes} bytes")
        N = actions.shape[1]
        if rewards.shape[1] != N or dones.shape[1] != N:
            raise ValueError("actions, rewards and dones must be [P*E, n_drones]")
        E = n // self.members
        _check(self.L, self.L.drl_pop_replay_add(ctypes.byref(self.desc), self.members, ctypes.byref(self._c),
                                                 self.cursor, E, _vp(code_prev.data_ptr()), _vp(code.data_ptr()),
                                                 _vp(actions.data_ptr()), _vp(rewards.data_ptr()),
                                                 _vp(dones.data_ptr()), N, _stream(dev)))
        self.cursor = (self.cursor + E) % self.capacity
        self.size = min(self.size + E, self.capacity)

    def ring(self, m: int) -> dict:
        """Views of member m's ring (obs, next_obs, actions, rewards, dones)."""
        s = slice(m * self.capacity, (m + 1) * self.capacity)
        return dict(obs=self.obs[s], next_obs=self.next_obs[s], actions=self.actions[s], rewards=self.rewards[s],
                    dones=self.dones[s])


DOUBLE_CONV_POP_REFUSAL = ("double_dqn: a conv population (ConvPopulationDQN) trains the max rule only; Double DQN "
                           "is implemented for dense populations (PopulationDQN)")
DOUBLE_PER_POP_REFUSAL = ("double_dqn: a prioritized population (PrioritizedPopulationDQN) trains the max rule only; "
                          "Double DQN is implemented for uniform dense populations (PopulationDQN)")


class PopulationDQN:
    """P dense DQN agents in one device allocation: member m's block is laid
    out as LargeBatchDQNLearner's / WideDQNLearner's (four parameter sets,
    counters, scratch for `max_batch`), a hyperparameter record per member
    beside them (uploaded once: `train` passes no host hyperparameters).

    hps: a DQNHParams per member (batch in [1, max_batch]; max_batch
    defaults to the largest).  hidden: 1-3 widths, multiples of 8 up to 256.
    seeds: member m's initialisation seed (the online net from seeds[m], the
    target net from seeds[m] + 1, as `train` does); or `online` / `target`:
    per member ([weights], [biases]) in torch layout.

    A member whose hp.double_dqn is set trains with the Double DQN target
    (drl_pop_double_train: the rule is a device byte per member, `double_mask`,
    so both rules share one launch chain); with no such member `train` is
    drl_pop_train."""

    _double_refusal = None  # a subclass whose chain keeps the max rule: the message it refuses hp.double_dqn with

    def __init__(self, in_features: int, hidden: Sequence[int], hps: Sequence[DQNHParams], envs_per_member: int,
                 n_actions: int = NUM_ACTIONS, device=None, seeds: Optional[Sequence[int]] = None,
                 max_batch: Optional[int] = None, online=None, target=None, guard_bytes: int = 0):
        self.L = _bind_pop(_bind(lib()))
        self.hps = list(hps)
        if self._double_refusal and any(hp.double_dqn for hp in self.hps):
            raise ValueError(self._double_refusal)
        self.members = len(self.hps)
        self.E = int(envs_per_member)
        self.in_features, self.hidden, self.n_actions = int(in_features), tuple(int(w) for w in hidden), int(n_actions)
        self.desc = pop_desc(self.in_features, self.hidden, self.n_actions)
        self.max_batch = int(max_batch) if max_batch is not None else max([hp.batch for hp in self.hps] or [1])
        lay = DrlPopLayout()
        if self.L.drl_pop_layout_query(ctypes.byref(self.desc), self.members, self.max_batch, ctypes.byref(lay)):
            raise ValueError(self.L.drl_last_error().decode())
        if self.E < 1:
            raise ValueError("envs_per_member must be >= 1")
        for m, hp in enumerate(self.hps):
            if not 1 <= hp.batch <= self.max_batch:
                raise ValueError(f"member {m}: batch must be in [1, max_batch={self.max_batch}]")
        self.layout = lay
        self.window = round((self.in_features / 6) ** 0.5)
        self.code_bytes = int(self.L.drl_policy_code_bytes((self.window - 1) // 2))
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # (guard_bytes behind the population: tests fill them and check that nothing writes there)
        self._alloc = torch.zeros(lay.bytes + int(guard_bytes), dtype=torch.uint8, device=self.device)
        self.block = self._alloc[:lay.bytes]
        self._f32 = self.block.view(torch.float32)
        sizes = [self.in_features, *self.hidden, self.n_actions]
        self.shapes = [((sizes[i + 1], sizes[i]), (sizes[i + 1],)) for i in range(len(sizes) - 1)]
        nl = len(self.shapes)
        seeds = list(seeds) if seeds is not None else [0] * self.members
        if len(seeds) != self.members:
            raise ValueError("seeds: one per member")

        def fresh(seed):
            g = torch.Generator().manual_seed(int(seed))
            return ([flax_kernel_init(ws, 2.0 if l < nl - 1 else 1.0, g) for l, (ws, _) in enumerate(self.shapes)],
                    [torch.zeros(bs) for _, bs in self.shapes])

        for m in range(self.members):
            on = online[m] if online is not None else fresh(seeds[m])
            tg = target[m] if target is not None else fresh(seeds[m] + 1)
            for which, (ws, bs) in (("online", on), ("target", tg)):
                for l, (w, b) in enumerate(self.params(which, m)):
                    w.copy_(torch.as_tensor(ws[l]).to(self.device, torch.float32))
                    b.copy_(torch.as_tensor(bs[l]).to(self.device, torch.float32))
        # drl_dqn_counters.epsilon of every member: a strided view of the block
        self.epsilon = self._f32.as_strided((self.members,), (lay.member_stride // 4,),
                                            (lay.member.counters_off + 8) // 4)
        self._hp = (DrlDqnHParams * self.members)(*[hp.c() for hp in self.hps])
        # the members' TD rule: a device byte each (nonzero: Double DQN), read by drl_pop_double_train's kernels
        self.double_mask = torch.tensor([1 if hp.double_dqn else 0 for hp in self.hps], dtype=torch.uint8,
                                        device=self.device)
        self._any_double = any(hp.double_dqn for hp in self.hps)
        self.restart()

    # ---------------------------------------------------------------- state --
    def restart(self):
        """drl_pop_init: every member's Adam moments and counters from zero,
        epsilon = its epsilon_start; the parameters are kept."""
        eps = (ctypes.c_float * self.members)(*[float(hp.epsilon_start) for hp in self.hps])
        if self.L.drl_pop_init(ctypes.byref(self.desc), self.members, self.max_batch, self._hp, eps,
                               _vp(self.block.data_ptr()), _stream(self.device)):
            raise ValueError(self.L.drl_last_error().decode())

    def member_block(self, m: int) -> torch.Tensor:
        """Member m's agent block (uint8 view): drl_dqn_large_layout_query's layout."""
        if not 0 <= m < self.members:
            raise IndexError("member out of range")
        s = self.layout.member_stride
        return self.block[m * s:m * s + self.layout.member.bytes]

    def params(self, which: str, m: int):
        """[(W [out][in], b [out])] views of member m's parameter set
        ("online", "target", "m", "v")."""
        if which not in SETS:
            raise ValueError(f"which must be one of {SETS}")
        lay = self.layout.member
        off = getattr(lay, which + "_off")
        s = self.member_block(m)[off:off + 4 * lay.n_params].view(torch.float32)
        out = []
        for l, (ws, bs) in enumerate(self.shapes):
            wo, bo = lay.weight_off[l], lay.bias_off[l]
            out.append((s[wo:wo + ws[0] * ws[1]].view(ws), s[bo:bo + bs[0]]))
        return out

    def counters(self, m: int) -> dict:
        """Host copy of member m's device counters (synchronises)."""
        c = self.member_block(m)[self.layout.member.counters_off:self.layout.member.counters_off + 64].cpu()
        f, i, d = c.view(torch.float32), c.view(torch.int32), c[16:32].view(torch.float64)
        return {"step": int(i[0]), "count": int(i[1]), "epsilon": float(f[2]), "loss": float(f[3]),
                "beta1_pow": float(d[0]), "beta2_pow": float(d[1]), "trained": int(i[9])}

    # ----------------------------------------------------------------- step --
    def act(self, code: torch.Tensor, step: int, seed: int = 0, env_offset: int = 0,
            actions: Optional[torch.Tensor] = None, synth=(0, 0), greedy: bool = False,
            q_out: Optional[torch.Tensor] = None, n_drones: int = 1) -> torch.Tensor:
        """Column 0 of actions [P*E, n_drones]: each env's epsilon-greedy
        action from its member's online net and device epsilon (greedy: no
        exploration, whatever epsilon holds); columns 1..: the synthetic
        stream synth=(seed, step) (BatchedDeliveryDrones.synth_actions).
        code: uint8 [P*E, code_bytes].  q_out: float32 [P*E, n_actions]."""
        n = self.members * self.E
        _on(code, self.device, torch.uint8, "code")
        if tuple(code.shape) != (n, self.code_bytes) or not code.is_contiguous():
            raise ValueError(f"code must be a contiguous uint8 [{n}, {self.code_bytes}] tensor")
        if actions is None:
            actions = torch.empty((n, n_drones), dtype=torch.int32, device=self.device)
        _on(actions, self.device, torch.int32, "actions")
        if actions.dim() != 2 or actions.shape[0] != n or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous int32 [{n}, n_drones] tensor")
        if q_out is not None:
            _on(q_out, self.device, torch.float32, "q_out")
            if tuple(q_out.shape) != (n, self.n_actions) or not q_out.is_contiguous():
                raise ValueError(f"q_out must be a contiguous float32 [{n}, {self.n_actions}] tensor")
        _check(self.L, self.L.drl_pop_act(
            ctypes.byref(self.desc), self.members, self.max_batch, _vp(self.block.data_ptr()), _vp(code.data_ptr()),
            self.E, int(bool(greedy)), seed & (2**64 - 1), int(step), int(env_offset), _vp(actions.data_ptr()),
            actions.shape[1], synth[0] & (2**64 - 1), int(synth[1]),
            None if q_out is None else _vp(q_out.data_ptr()), _stream(self.device)))
        return actions

    def train(self, replay: PopulationReplay):
        """One learner block (train_jax.py:68-98) of every member on its ring:
        member m trains iff replay.size >= its batch (decided on the device)."""
        if replay.obs.device != self.device or replay.members != self.members:
            raise ValueError("the replay must be on the population's device and hold one ring per member")
        if self._any_double:
            _check(self.L, self.L.drl_pop_double_train(ctypes.byref(self.desc), self.members, self.max_batch,
                                                       _vp(self.block.data_ptr()), ctypes.byref(replay._c),
                                                       replay.size, _vp(self.double_mask.data_ptr()),
                                                       _stream(self.device)))
            return
        _check(self.L, self.L.drl_pop_train(ctypes.byref(self.desc), self.members, self.max_batch,
                                            _vp(self.block.data_ptr()), ctypes.byref(replay._c), replay.size,
                                            _stream(self.device)))

    def sample_slots(self, size: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int64 [P, max_batch]: the slots member m's next train step draws in
        its first batch_m entries, -1 behind them (stream-ordered, no sync)."""
        if out is None:
            out = torch.empty((self.members, self.max_batch), dtype=torch.int64, device=self.device)
        _on(out, self.device, torch.int64, "out")
        if tuple(out.shape) != (self.members, self.max_batch) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int64 [{self.members}, {self.max_batch}] tensor")
        _check(self.L, self.L.drl_pop_sample_rows(ctypes.byref(self.desc), self.members, self.max_batch,
                                                  _vp(self.block.data_ptr()), int(size), _vp(out.data_ptr()),
                                                  _stream(self.device)))
        return out

    def check_errors(self):
        """Synchronise and raise if a member's online parameters are no longer
        finite (the launches wait for nothing, so there is no timeout to
        report)."""
        torch.cuda.synchronize(self.device)
        for m in range(self.members):
            off = self.layout.member.online_off
            s = self.member_block(m)[off:off + 4 * self.layout.member.n_params].view(torch.float32)
            if not bool(torch.isfinite(s).all()):
                raise DroneRLError(f"population member {m}: the online parameters are not finite")

    # ------------------------------------------------------------- members --
    def member_net(self, m: int, input: str = "obs"):
        """A QNetwork (widths up to 128) or WideQNetwork loaded with member
        m's online weights: what train.evaluate and the line-up evaluator
        take."""
        cls = WideQNetwork if is_wide(self.hidden) else QNetwork
        net = cls(self.in_features, self.hidden, n_actions=self.n_actions, device=self.device, input=input)
        net.load(*zip(*self.params("online", m)))
        return net

    def save(self, m: int, path: str, format: str = "torch", **kw):
        """Member m's online net as train_jax.py:238-244 saves a trained agent
        (checkpoint.save_dense)."""
        from .checkpoint import save_dense
        ws, bs = zip(*self.params("online", m))
        save_dense(path, ws, bs, (self.window, self.window, 6), format=format, **kw)


class DrlConvPopLayout(ctypes.Structure):
    _fields_ = [("member", DrlConvnetDqnLayout), ("member_stride", ctypes.c_int64), ("hparams_off", ctypes.c_int64),
                ("hparams_stride", ctypes.c_int64), ("bytes", ctypes.c_int64), ("members", ctypes.c_int32),
                ("max_batch", ctypes.c_int32)]


def _bind_convpop(L):
    if getattr(L, "_convpop_ready", False):
        return L
    i32, i64, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    D, R = ctypes.POINTER(DrlConvnetDesc), ctypes.POINTER(DrlReplay)
    sig = {
        "drl_convpop_layout_query": [D, i32, i32, ctypes.POINTER(DrlConvPopLayout)],
        "drl_convpop_init": [D, i32, i32, ctypes.POINTER(DrlDqnHParams), ctypes.POINTER(ctypes.c_float), _vp, _vp],
        "drl_convpop_act": [D, i32, i32, _vp, _vp, i64, i32, u64, u64, i64, _vp, i32, u64, u64, _vp, _vp],
        "drl_convpop_train": [D, i32, i32, _vp, R, i64, _vp],
        "drl_convpop_sample_rows": [D, i32, i32, _vp, i64, _vp, _vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = ctypes.c_int
    L._convpop_ready = True
    return L


class ConvPopulationDQN(PopulationDQN):
    """P conv DQN agents in one device allocation (drl_convpop_*;
    dronerl_amd/csrc/convpop/): PopulationDQN's surface for a ConvQNetwork
    architecture on the policy code.  Member m's block is laid out as
    LargeBatchConvDQNLearner's at `max_batch`; its arithmetic is that
    learner's bit for bit, whoever shares the population.

    The act is an f32 forward by the learner's own per-layer code on the
    member's online set (its Q is the learner's Q bit for bit; no packed image
    exists and nothing is re-packed after a train step).  ConvQNetwork's MFMA
    act agrees with it to ~1e-5, not bit for bit, so a member reproduces under
    this API, not necessarily under `train()`.

    obs_shape (W, W, 6) with W in 5, 7, 9; conv_layers / dense_layers as
    ConvQNetwork takes them.  seeds: member m's online net from seeds[m], its
    target net from seeds[m] + 1, as `train` initialises a conv agent; or
    `online` / `target`: per member ([weights], [biases]) in forward order
    (conv layers [out][in][k][k], then dense [out][in], the Q head last)."""

    _double_refusal = DOUBLE_CONV_POP_REFUSAL

    def __init__(self, obs_shape, conv_layers, dense_layers: Sequence[int], hps: Sequence[DQNHParams],
                 envs_per_member: int, n_actions: int = NUM_ACTIONS, device=None,
                 seeds: Optional[Sequence[int]] = None, max_batch: Optional[int] = None, online=None, target=None,
                 guard_bytes: int = 0):
        self.L = _bind_convpop(_bind_pop(_bind(_bind_convnet(lib()))))
        self.hps = list(hps)
        if any(hp.double_dqn for hp in self.hps):
            raise ValueError(self._double_refusal)
        self.members = len(self.hps)
        self.E = int(envs_per_member)
        self.obs_shape = tuple(int(v) for v in obs_shape)
        self.desc = convnet_desc(self.obs_shape, conv_layers, dense_layers, n_actions, "code")
        self.conv_layers = tuple({"out_channels": int(c.out_channels), "kernel_size": int(c.kernel_size),
                                  "stride": int(c.stride), "padding": int(c.padding)}
                                 for c in self.desc.conv[:self.desc.n_conv])
        self.dense_layers, self.n_actions = tuple(int(w) for w in dense_layers), int(n_actions)
        self.max_batch = int(max_batch) if max_batch is not None else max([hp.batch for hp in self.hps] or [1])
        lay = DrlConvPopLayout()
        if self.L.drl_convpop_layout_query(ctypes.byref(self.desc), self.members, self.max_batch, ctypes.byref(lay)):
            raise ValueError(self.L.drl_last_error().decode())
        if self.E < 1:
            raise ValueError("envs_per_member must be >= 1")
        for m, hp in enumerate(self.hps):
            if not 1 <= hp.batch <= self.max_batch:
                raise ValueError(f"member {m}: batch must be in [1, max_batch={self.max_batch}]")
        self.layout = lay
        self.window = self.obs_shape[0]
        self.in_features = self.window * self.window * 6
        self.code_bytes = int(self.L.drl_policy_code_bytes((self.window - 1) // 2))
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._alloc = torch.zeros(lay.bytes + int(guard_bytes), dtype=torch.uint8, device=self.device)
        self.block = self._alloc[:lay.bytes]
        self._f32 = self.block.view(torch.float32)
        self.shapes, side, cin = [], self.window, 6
        for c in self.conv_layers:
            k, co = c["kernel_size"], c["out_channels"]
            self.shapes.append(((co, cin, k, k), (co,)))
            side, cin = (side + 2 * c["padding"] - k) // c["stride"] + 1, co
        sizes = [side * side * cin, *self.dense_layers, self.n_actions]
        self.shapes += [((sizes[i + 1], sizes[i]), (sizes[i + 1],)) for i in range(len(sizes) - 1)]
        seeds = list(seeds) if seeds is not None else [0] * self.members
        if len(seeds) != self.members:
            raise ValueError("seeds: one per member")

        def fresh(seed):  # (ConvQNetwork's own draw order: flax Conv / Dense lecun_normal, zero biases)
            g = torch.Generator().manual_seed(int(seed))
            return ([flax_kernel_init((ws[0], int(torch.Size(ws[1:]).numel())), 1.0, g).reshape(ws)
                     for ws, _ in self.shapes], [torch.zeros(bs) for _, bs in self.shapes])

        for m in range(self.members):
            on = online[m] if online is not None else fresh(seeds[m])
            tg = target[m] if target is not None else fresh(seeds[m] + 1)
            for which, (ws, bs) in (("online", on), ("target", tg)):
                if len(ws) != len(self.shapes) or len(bs) != len(self.shapes):
                    raise ValueError(f"member {m} {which}: layer count mismatch")
                for l, (w, b) in enumerate(self.params(which, m)):
                    w.copy_(torch.as_tensor(ws[l]).to(self.device, torch.float32))
                    b.copy_(torch.as_tensor(bs[l]).to(self.device, torch.float32))
        self.epsilon = self._f32.as_strided((self.members,), (lay.member_stride // 4,),
                                            (lay.member.counters_off + 8) // 4)
        self._hp = (DrlDqnHParams * self.members)(*[hp.c() for hp in self.hps])
        self.restart()

    def restart(self):
        """drl_convpop_init: every member's Adam moments and counters from
        zero, epsilon = its epsilon_start; the parameters are kept."""
        eps = (ctypes.c_float * self.members)(*[float(hp.epsilon_start) for hp in self.hps])
        if self.L.drl_convpop_init(ctypes.byref(self.desc), self.members, self.max_batch, self._hp, eps,
                                   _vp(self.block.data_ptr()), _stream(self.device)):
            raise ValueError(self.L.drl_last_error().decode())

    def params(self, which: str, m: int):
        """[(W, b)] views of member m's parameter set ("online", "target",
        "m", "v") in ConvDQNLearner.params' order and torch layouts."""
        if which not in SETS:
            raise ValueError(f"which must be one of {SETS}")
        lay = self.layout.member
        off = getattr(lay, which + "_off")
        s = self.member_block(m)[off:off + 4 * lay.n_params].view(torch.float32)
        out = []
        for l, (ws, bs) in enumerate(self.shapes):
            wo, bo = lay.weight_off[l], lay.bias_off[l]
            out.append((s[wo:wo + int(torch.Size(ws).numel())].view(ws), s[bo:bo + bs[0]]))
        return out

    def act(self, code: torch.Tensor, step: int, seed: int = 0, env_offset: int = 0,
            actions: Optional[torch.Tensor] = None, synth=(0, 0), greedy: bool = False,
            q_out: Optional[torch.Tensor] = None, n_drones: int = 1) -> torch.Tensor:
        """PopulationDQN.act's arguments and result (drl_convpop_act)."""
        n = self.members * self.E
        _on(code, self.device, torch.uint8, "code")
        if tuple(code.shape) != (n, self.code_bytes) or not code.is_contiguous():
            raise ValueError(f"code must be a contiguous uint8 [{n}, {self.code_bytes}] tensor")
        if actions is None:
            actions = torch.empty((n, n_drones), dtype=torch.int32, device=self.device)
        _on(actions, self.device, torch.int32, "actions")
        if actions.dim() != 2 or actions.shape[0] != n or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous int32 [{n}, n_drones] tensor")
        if q_out is not None:
            _on(q_out, self.device, torch.float32, "q_out")
            if tuple(q_out.shape) != (n, self.n_actions) or not q_out.is_contiguous():
                raise ValueError(f"q_out must be a contiguous float32 [{n}, {self.n_actions}] tensor")
        _check(self.L, self.L.drl_convpop_act(
            ctypes.byref(self.desc), self.members, self.max_batch, _vp(self.block.data_ptr()), _vp(code.data_ptr()),
            self.E, int(bool(greedy)), seed & (2**64 - 1), int(step), int(env_offset), _vp(actions.data_ptr()),
            actions.shape[1], synth[0] & (2**64 - 1), int(synth[1]),
            None if q_out is None else _vp(q_out.data_ptr()), _stream(self.device)))
        return actions

    def train(self, replay: PopulationReplay):
        """One learner block (train_jax.py:68-98, network_type conv) of every
        member on its ring: member m trains iff replay.size >= its batch
        (decided on the device)."""
        if replay.obs.device != self.device or replay.members != self.members:
            raise ValueError("the replay must be on the population's device and hold one ring per member")
        _check(self.L, self.L.drl_convpop_train(ctypes.byref(self.desc), self.members, self.max_batch,
                                                _vp(self.block.data_ptr()), ctypes.byref(replay._c), replay.size,
                                                _stream(self.device)))

    def sample_slots(self, size: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """PopulationDQN.sample_slots (drl_convpop_sample_rows)."""
        if out is None:
            out = torch.empty((self.members, self.max_batch), dtype=torch.int64, device=self.device)
        _on(out, self.device, torch.int64, "out")
        if tuple(out.shape) != (self.members, self.max_batch) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int64 [{self.members}, {self.max_batch}] tensor")
        _check(self.L, self.L.drl_convpop_sample_rows(ctypes.byref(self.desc), self.members, self.max_batch,
                                                      _vp(self.block.data_ptr()), int(size), _vp(out.data_ptr()),
                                                      _stream(self.device)))
        return out

    def member_net(self, m: int, input: str = "obs"):
        """A ConvQNetwork loaded with member m's online weights: what
        train.evaluate and the line-up evaluator take."""
        net = ConvQNetwork(self.obs_shape, self.conv_layers, self.dense_layers, n_actions=self.n_actions,
                           device=self.device, input=input)
        ws, bs = zip(*self.params("online", m))
        nc = len(self.conv_layers)
        net.load(ws[:nc], bs[:nc], ws[nc:], bs[nc:])
        return net

    def save(self, m: int, path: str, format: str = "torch", **kw):
        """Member m's online net as train_jax.py:238-244 saves a trained conv
        agent (checkpoint.save_conv)."""
        from .checkpoint import save_conv
        ws, bs = zip(*self.params("online", m))
        nc = len(self.conv_layers)
        kw.setdefault("conv_layers", self.conv_layers)
        save_conv(path, ws[:nc], bs[:nc], ws[nc:], bs[nc:], self.obs_shape, format=format, **kw)


class DrlPopPerLayout(ctypes.Structure):
    _fields_ = [("member", DrlPerLayout), ("member_stride", ctypes.c_int64), ("hparams_off", ctypes.c_int64),
                ("hparams_stride", ctypes.c_int64), ("bytes", ctypes.c_int64), ("members", ctypes.c_int32),
                ("max_batch", ctypes.c_int32)]


def _bind_pop_per(L):
    if getattr(L, "_pop_per_ready", False):
        return L
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    D, R = ctypes.POINTER(DrlWidenetDesc), ctypes.POINTER(DrlReplay)
    sig = {
        "drl_pop_per_layout_query": [i32, i64, i32, ctypes.POINTER(DrlPopPerLayout)],
        "drl_pop_per_init": [i32, i64, i32, ctypes.POINTER(DrlPerHParams), _vp, _vp],
        "drl_pop_per_mark_new": [i32, i64, i32, _vp, i64, i64, _vp],
        "drl_pop_per_rebuild": [i32, i64, i32, _vp, _vp],
        "drl_pop_per_sample": [D, i32, i32, _vp, _vp, i64, i64, _vp],
        "drl_pop_per_train": [D, i32, i32, _vp, R, i64, _vp, _vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = ctypes.c_int
    L._pop_per_ready = True
    return L


PER_KEYS = ("alpha", "beta0", "beta_steps", "eps")


def per_record(per: Optional[dict] = None) -> dict:
    """A member's PER hyperparameters (dqn.PrioritizedReplay's keywords and
    defaults), validated by name."""
    rec = dict(alpha=0.6, beta0=0.4, beta_steps=0, eps=1e-6)
    for k, v in (per or {}).items():
        if k not in PER_KEYS:
            raise ValueError(f"per: {k} is not one of {', '.join(PER_KEYS)}")
        rec[k] = v
    if not rec["alpha"] >= 0:
        raise ValueError("alpha must be >= 0")
    if not 0 <= rec["beta0"] <= 1:
        raise ValueError("beta0 must be in [0, 1]")
    if rec["beta_steps"] < 0:
        raise ValueError("beta_steps must be >= 0")
    if not rec["eps"] >= 0:
        raise ValueError("eps must be >= 0")
    return dict(alpha=float(rec["alpha"]), beta0=float(rec["beta0"]), beta_steps=int(rec["beta_steps"]),
                eps=float(rec["eps"]))


class PrioritizedPopulationReplay:
    """Proportional prioritized replay around a PopulationReplay, which stays
    as it is: a priority sum tree per member over its ring, in one allocation
    (drl_pop_per_*; include/dronerl.h describes the block), each member with
    its own alpha, beta0, beta_steps and eps.  `add` is the population's add
    followed by drl_pop_per_mark_new for the same cursor and count: the new
    rows enter every member's tree with that member's largest priority so far.

    pers: one dict alpha / beta0 / beta_steps / eps per member (missing keys:
    dqn.PrioritizedReplay's defaults).  max_batch: the population's.  Views of
    member m's block: tree(m) (f32 [2P]), pmax(m), wmax(m) (f32 [1]),
    slots(m) (int64 [max_batch]), weights(m) and abs_td(m) (f32 [max_batch]);
    a member's step fills the first batch_m entries."""

    def __init__(self, replay: PopulationReplay, pers: Sequence[dict], max_batch: int, guard_bytes: int = 0):
        if not isinstance(replay, PopulationReplay):
            raise ValueError("PrioritizedPopulationReplay wraps a population.PopulationReplay")
        self.replay, self.L = replay, _bind_pop_per(replay.L)
        self.pers = [per_record(p) for p in pers]
        if len(self.pers) != replay.members:
            raise ValueError("pers: one dict of PER hyperparameters per member")
        self.max_batch = int(max_batch)
        lay = DrlPopPerLayout()
        if self.L.drl_pop_per_layout_query(replay.members, replay.capacity, self.max_batch, ctypes.byref(lay)):
            raise ValueError(self.L.drl_last_error().decode())
        self.layout = lay
        dev = replay.obs.device
        self._alloc = torch.zeros(lay.bytes + int(guard_bytes), dtype=torch.uint8, device=dev)
        self.block = self._alloc[:lay.bytes]
        self._hp = (DrlPerHParams * replay.members)(*[DrlPerHParams(p["alpha"], p["beta0"], p["beta_steps"], p["eps"])
                                                      for p in self.pers])
        _check(self.L, self.L.drl_pop_per_init(replay.members, replay.capacity, self.max_batch, self._hp,
                                               _vp(self.block.data_ptr()), _stream(dev)))
        if replay.size:  # the rows written before the trees existed: the ring's contents as wrapped
            self._mark(0 if replay.size < replay.capacity else replay.cursor, replay.size)

    members = property(lambda self: self.replay.members)
    capacity = property(lambda self: self.replay.capacity)
    size = property(lambda self: self.replay.size)
    cursor = property(lambda self: self.replay.cursor)
    obs = property(lambda self: self.replay.obs)

    def ring(self, m: int) -> dict:
        return self.replay.ring(m)

    def _mark(self, cursor: int, count: int):
        _check(self.L, self.L.drl_pop_per_mark_new(self.members, self.capacity, self.max_batch,
                                                   _vp(self.block.data_ptr()), int(cursor), int(count),
                                                   _stream(self.replay.obs.device)))

    def add(self, code_prev: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, code: torch.Tensor,
            dones: torch.Tensor):
        """PopulationReplay.add, then the new rows' leaves = the member's pmax."""
        cursor = self.replay.cursor
        self.replay.add(code_prev, actions, rewards, code, dones)
        self._mark(cursor, code.shape[0] // self.members)

    def rebuild(self):
        """Every internal node of every member's tree from its leaves (drl_pop_per_rebuild)."""
        _check(self.L, self.L.drl_pop_per_rebuild(self.members, self.capacity, self.max_batch,
                                                  _vp(self.block.data_ptr()), _stream(self.replay.obs.device)))

    def _view(self, m: int, off: int, n: int, dt, size: int) -> torch.Tensor:
        if not 0 <= m < self.members:
            raise IndexError("member out of range")
        at = m * self.layout.member_stride + off
        return self.block[at:at + n * size].view(dt)

    def member_block(self, m: int) -> torch.Tensor:
        """Member m's prioritized block (uint8 view): drl_per_layout_query's layout."""
        return self._view(m, 0, self.layout.member.bytes, torch.uint8, 1)

    def tree(self, m: int) -> torch.Tensor:
        return self._view(m, self.layout.member.tree_off, 2 * self.layout.member.leaves, torch.float32, 4)

    def pmax(self, m: int) -> torch.Tensor:
        return self._view(m, self.layout.member.pmax_off, 1, torch.float32, 4)

    def wmax(self, m: int) -> torch.Tensor:
        return self._view(m, self.layout.member.wmax_off, 1, torch.float32, 4)

    def slots(self, m: int) -> torch.Tensor:
        return self._view(m, self.layout.member.slots_off, self.max_batch, torch.int64, 8)

    def weights(self, m: int) -> torch.Tensor:
        return self._view(m, self.layout.member.weights_off, self.max_batch, torch.float32, 4)

    def abs_td(self, m: int) -> torch.Tensor:
        return self._view(m, self.layout.member.absd_off, self.max_batch, torch.float32, 4)


class PrioritizedPopulationDQN(PopulationDQN):
    """PopulationDQN on prioritized rows (drl_pop_per_train): the same block,
    act and launch chain; `train(replay)` takes a PrioritizedPopulationReplay
    and every member that holds a batch rebuilds its tree, draws by priority,
    trains with each row's importance weight on its squared error and on the
    Q head's delta, and writes (|td error| + eps) ** alpha back to the drawn
    slots -- PrioritizedDQNLearner's step bit for bit at the widths both take,
    whoever shares the population; stream-ordered, graph-capturable, a launch
    count that does not depend on the number of members."""

    _double_refusal = DOUBLE_PER_POP_REFUSAL

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.L = _bind_pop_per(self.L)

    def _check_replay(self, replay):
        if not isinstance(replay, PrioritizedPopulationReplay):
            raise ValueError("PrioritizedPopulationDQN.train takes a PrioritizedPopulationReplay")
        if replay.obs.device != self.device or replay.members != self.members:
            raise ValueError("the replay must be on the population's device and hold one ring per member")
        if replay.max_batch != self.max_batch:
            raise ValueError(f"the prioritized replay is laid out for max_batch {replay.max_batch}, the population "
                             f"for {self.max_batch}")

    def train(self, replay: PrioritizedPopulationReplay):
        """One prioritized learner block of every member on its ring: member
        m trains iff replay.size >= its batch (decided on the device)."""
        self._check_replay(replay)
        _check(self.L, self.L.drl_pop_per_train(ctypes.byref(self.desc), self.members, self.max_batch,
                                                _vp(self.block.data_ptr()), ctypes.byref(replay.replay._c),
                                                replay.size, _vp(replay.block.data_ptr()), _stream(self.device)))

    def sample(self, replay: PrioritizedPopulationReplay):
        """drl_pop_per_sample from the trees as they stand (replay.rebuild()
        first): the slots, weights and wmax of every member that holds a
        batch, for the step its counters hold."""
        self._check_replay(replay)
        _check(self.L, self.L.drl_pop_per_sample(ctypes.byref(self.desc), self.members, self.max_batch,
                                                 _vp(self.block.data_ptr()), _vp(replay.block.data_ptr()),
                                                 replay.capacity, replay.size, _stream(self.device)))


@dataclass
class PopulationResult:
    env: object
    pop: PopulationDQN
    replay: PopulationReplay
    steps: int
    agent_steps_per_s: float


def train_population(params: EnvParams, members: Sequence[DQNHParams], envs_per_member: int, num_steps: int,
                     hidden: Sequence[int] = (128, 64), reset_env_every: int = 100, memory_size: int = 100_000,
                     seed: int = 0, env_offset: int = 0, action_seed: int = 2024, act_seed: int = 7, device=None,
                     seeds: Optional[Sequence[int]] = None, on_step=None, network_type: str = "dense",
                     conv_layers=None, conv_dense_layers: Sequence[int] = (), per: Optional[Sequence[dict]] = None,
                     **pop_kw) -> PopulationResult:
    """`train`'s loop for a population: per step the population act, one env
    step over all P*E envs writing drone 0's next policy code, the add into
    the members' rings, the members' learner blocks, and a reset of every env
    when step % reset_env_every == 0 (train_jax.py:99-113).  members: a
    DQNHParams each; seeds: each member's initialisation seed (default
    `seed` for all).  on_step(t, pop, replay, acts, rewards, dones): called
    between step t's add and its train (tests).  network_type "conv": a
    ConvPopulationDQN of conv_layers (default train_jax.py's one 3x3 layer of
    8 channels, padding 1) and conv_dense_layers; `hidden` is then unused.
    per: one dict alpha / beta0 / beta_steps / eps per member: a
    PrioritizedPopulationDQN on a PrioritizedPopulationReplay (dense nets
    only); None: uniform replay."""
    from .env import BatchedDeliveryDrones
    if num_steps < 1 or reset_env_every < 1:
        raise ValueError("num_steps and reset_env_every must be >= 1")
    if network_type not in ("dense", "conv"):
        raise ValueError("network_type must be 'dense' or 'conv'")
    members = list(members)
    if per is not None:
        if network_type == "conv":
            raise ValueError("train_population(per=...) with network_type='conv' is not implemented: a prioritized "
                             "population trains dense nets only")
        per = list(per)
        if len(per) != len(members):
            raise ValueError("per: one dict of PER hyperparameters per member")
    P, E = len(members), int(envs_per_member)
    env = BatchedDeliveryDrones(params, P * E, device=device, env_offset=env_offset)
    env.reset(seed=seed)
    dev, N, r = env.device, env.n_drones, params.window_radius
    D = (2 * r + 1) ** 2 * 6
    seeds = seeds if seeds is not None else [seed] * P
    if network_type == "conv":
        from .checkpoint import TRAIN_JAX_CONV_LAYERS
        W = 2 * r + 1
        pop = ConvPopulationDQN((W, W, 6), conv_layers if conv_layers is not None else TRAIN_JAX_CONV_LAYERS,
                                tuple(conv_dense_layers), members, E, device=dev, seeds=seeds, **pop_kw)
    elif per is not None:
        pop = PrioritizedPopulationDQN(D, hidden, members, E, device=dev, seeds=seeds, **pop_kw)
    else:
        pop = PopulationDQN(D, hidden, members, E, device=dev, seeds=seeds, **pop_kw)
    rb = PopulationReplay(P, memory_size, r, device=dev)
    if per is not None:
        rb = PrioritizedPopulationReplay(rb, per, pop.max_batch)
    code = [env.new_code(), env.new_code()]
    env.get_code(out=code[0])
    acts = torch.empty((P * E, N), dtype=torch.int32, device=dev)
    rew = torch.empty((P * E, N), dtype=torch.float32, device=dev)
    don = torch.empty((P * E, N), dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(num_steps):
        b, nb = t & 1, (t + 1) & 1
        pop.act(code[b], t, seed=act_seed, env_offset=env.env_offset, actions=acts, synth=(action_seed, t))
        env.step(acts, rewards=rew, dones=don, code=code[nb])
        rb.add(code[b], acts, rew, code[nb], don)
        if on_step is not None:
            on_step(t, pop, rb, acts, rew, don)
        pop.train(rb)
        if t % reset_env_every == 0:  # train_jax.py:101-113 (step 0 included)
            env.reset(seed=None)
            env.get_code(out=code[nb])
    e1.record()
    torch.cuda.synchronize(dev)
    env.check_errors()
    pop.check_errors()
    dt = e0.elapsed_time(e1) / 1e3
    return PopulationResult(env, pop, rb, num_steps, P * num_steps / dt)
