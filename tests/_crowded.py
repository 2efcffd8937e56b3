"""Crowded boards for tests/test_step_crowded.py: generated states on which a
single env-step respawns many items (numpy and the CPU oracle only; no GPU).

On boards made by ``reset`` and stepped with uniformly random actions very
little happens in one step, so the step kernel's respawn phase almost never
leaves the ring entries its lanes preload (DESIGN.md §4 phase 5).  The states
here are nearly full of ground objects, a third of the batteries are about to
run out and half the drones carry a packet, so one step crashes about a
quarter of its drones and a respawn needs many candidate cells.

Object codes: include/dronerl.h (the oracle's are the same).
"""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle
from oracle.oracle import MT, OracleMulti, Params

OBJ_EMPTY, OBJ_SKYSCRAPER, OBJ_STATION, OBJ_DROPZONE, OBJ_PACKET = 0, 2, 3, 4, 5
# share of the filled cells per object
OBJ_SHARE = ((OBJ_SKYSCRAPER, 0.25), (OBJ_STATION, 0.15), (OBJ_DROPZONE, 0.30), (OBJ_PACKET, 0.30))
E = 64          # envs per shape
STEPS = 6
# The committed seeds.  tests/test_step_crowded.py test 1 holds the input
# floors for both.  Seeds 0 and 1 miss one of them: at 128x128 the group is 64
# lanes wide (the LDS rule), so 64 entries are preloaded, and the share of
# env-steps past them is 0.46-0.54 over seeds 0-13 (0.49 / 0.50 at seeds 0 / 1)
# against a floor of 0.5; 9 and 11 give 0.54 and 0.52.
SEEDS = (9, 11)
CAND_SLOTS = 512  # ring entries per env (DRL_CAND_SLOTS)
# ACTION_TO_DIRECTION (env.py:26): LEFT DOWN RIGHT UP STAY as (dy, dx)
DIR = ((0, -1), (1, 0), (0, 1), (-1, 0), (0, 0))
EVENTS = ("delivery_and_battery_crash", "pickup_and_crash", "crash_while_carrying", "second_comer",
          "off_grid", "charging_at_100")


def step_cq(P: int) -> int:
    """Ring entries each step lane preloads (dronerl_internal.h step_cq with
    the default DRL_CQ_NARROW): P * step_cq(P) entries per env-step come
    without a second round trip."""
    return 2 if P <= 16 else 1


@dataclass(frozen=True)
class Shape:
    side: int
    n: int
    fill: float
    radius: int
    params: dict = field(default_factory=dict)

    @property
    def id(self) -> str:
        return f"g{self.side}_n{self.n}"

    def env_kwargs(self) -> dict:
        return dict(n_drones=self.n, grid_size=self.side, window_radius=self.radius, **self.params)

    def oracle_params(self) -> Params:
        return Params(side=self.side, n_drones=self.n, **self.params)


# Radius 3 stays on the four benchmark shapes (their compile-time instances);
# the others cover 1, 2, 5 and 8.
SHAPES = (
    Shape(5, 1, .60, 1),
    Shape(8, 4, .70, 3),
    Shape(6, 3, .55, 2, dict(discharge=0, charge=0)),
    Shape(16, 8, .90, 3),
    Shape(10, 8, .72, 5, dict(discharge=15, charge=30, pickup_reward=0.5, charge_reward=-0.25)),
    Shape(13, 11, .80, 8, dict(discharge=100, charge=1000)),
    Shape(32, 16, .95, 3),
    Shape(20, 16, .90, 2, dict(discharge=7, charge=33, delivery_reward=-2.5, crash_reward=1e6, pickup_reward=0.1)),
    Shape(33, 20, .95, 5),
    Shape(64, 32, .97, 3),
    Shape(24, 32, .85, 1, dict(discharge=1, charge=1)),
    Shape(26, 33, .85, 3),
    Shape(36, 64, .85, 2, dict(discharge=250, charge=100)),
    Shape(47, 5, .98, 8),
    Shape(128, 4, .99, 1),
)
BY_ID = {s.id: s for s in SHAPES}
BENCH_IDS = ("g8_n4", "g16_n8", "g32_n16", "g64_n32")


def generate(shape: Shape, seed: int) -> dict:
    """E crowded states and STEPS action sets, deterministic per (shape, seed)
    (RandomState: numpy freezes its streams)."""
    rs = np.random.RandomState([shape.side, shape.n, seed])
    G, N = shape.side, shape.n
    GG = G * G
    nfill = int(round(shape.fill * GG))
    codes = np.array([c for c, _ in OBJ_SHARE], np.uint8)
    share = np.array([s for _, s in OBJ_SHARE])
    ground = np.zeros((E, GG), np.uint8)
    order = np.zeros((E, N), np.int32)
    pos = np.zeros((E, N), np.int32)
    for e in range(E):
        ground[e, rs.permutation(GG)[:nfill]] = codes[rs.choice(len(codes), size=nfill, p=share)]
        free = np.flatnonzero(ground[e] != OBJ_SKYSCRAPER)
        pos[e] = free[rs.permutation(len(free))[:N]]
        order[e] = rs.permutation(N)
    low = rs.random_sample((E, N)) < 0.3
    charge = np.where(low, rs.randint(1, 21, (E, N)), rs.randint(1, 101, (E, N))).astype(np.int32)
    packet = rs.random_sample((E, N)) < 0.5
    actions = rs.randint(-5, 5, (STEPS, E, N)).astype(np.int32)  # negatives wrap (Python list index)
    return dict(ground=ground.reshape(E, G, G), order=order, y=pos // G, x=pos % G, charge=charge, packet=packet,
                actions=actions)


def entries_used(side: int, mt_before, mt_after, limit: int = 1 << 16) -> int:
    """Accepted (y, x) pairs between two getstate() word sets of one stream:
    the ring entries the env-step between them must consume."""
    before = np.ascontiguousarray(mt_before, np.uint32)
    after = np.ascontiguousarray(mt_after, np.uint32)
    m = MT()
    L = oracle.lib()
    L.orc_mt_set(m._p, before.ctypes.data_as(ctypes.c_void_p))
    now = np.zeros(625, np.uint32)
    pnow = now.ctypes.data_as(ctypes.c_void_p)
    randbelow, get, p = L.orc_randbelow, L.orc_mt_get, m._p
    pairs = 0
    while True:
        get(p, pnow)
        if now[624] == after[624] and np.array_equal(now, after):
            return pairs
        if pairs >= limit:
            raise AssertionError("mt_after is not reached from mt_before by randint pairs")
        randbelow(p, side)
        randbelow(p, side)
        pairs += 1


def count_events(shape: Shape, st: dict, actions: np.ndarray):
    """The combined events of one env-step, restated from env.py:124-195 on the
    state before the step: per-event counts over all envs and the crashed
    flags [E, N] (the test holds them against the oracle's dones)."""
    G, N = shape.side, shape.n
    p = shape.oracle_params()
    n = dict.fromkeys(EVENTS, 0)
    crashed = np.zeros((E, N), bool)
    for e in range(E):
        ground = st["ground"][e]
        claim = {}   # cell -> drone (new_drones)
        locs = set()  # crashed_drone_locations
        carry = st["packet"][e].copy()
        picked = set()
        for d in st["order"][e]:
            a = int(actions[e, d])
            dy, dx = DIR[a + 5 if a < 0 else a]
            y, x = int(st["y"][e, d]) + dy, int(st["x"][e, d]) + dx
            if not (0 <= y < G and 0 <= x < G):
                n["off_grid"] += 1
                crashed[e, d] = True
            elif (y, x) in claim:
                n["second_comer"] += 1  # the first-comer goes down with it (env.py:177-181)
                crashed[e, d] = True
                locs.add((y, x))
            else:
                claim[(y, x)] = d
        for (y, x), d in claim.items():
            obj, c = ground[y, x], int(st["charge"][e, d])
            dead = False
            if obj == OBJ_STATION:
                n["charging_at_100"] += c == 100
            else:
                dead = c - p.discharge <= 0
            if obj == OBJ_PACKET and not carry[d]:
                carry[d] = True
                picked.add(d)
            elif obj == OBJ_DROPZONE and carry[d]:
                carry[d] = False
                n["delivery_and_battery_crash"] += dead
            if dead or obj == OBJ_SKYSCRAPER:
                locs.add((y, x))
        for cell in locs:
            crashed[e, claim[cell]] = True
        n["pickup_and_crash"] += sum(bool(crashed[e, d]) for d in picked)
        n["crash_while_carrying"] += int((crashed[e] & carry).sum())
    return n, crashed


@dataclass
class Trajectory:
    shape: Shape
    seed: int
    init: dict
    actions: np.ndarray   # [STEPS, E, N]
    states: list          # STEPS + 1 oracle states (index t: after t steps)
    rewards: np.ndarray   # f64 [STEPS, E, N]
    dones: np.ndarray     # bool [STEPS, E, N]
    used: np.ndarray      # int [STEPS, E]: ring entries each env-step consumes
    error: str | None     # a NoFreeCell, if the oracle raised one

    def obs(self, t: int, k: int) -> np.ndarray:
        """The oracle's observation of drone indices 0..k-1 after t steps."""
        o = OracleMulti(self.shape.oracle_params(), E)
        s = self.states[t]
        o.set_state(s["ground"], s["order"], s["y"], s["x"], s["charge"], s["packet"], s["mt"])
        return o.obs(self.shape.radius, k)


def seeded_oracle(shape: Shape, seed: int, init: dict) -> OracleMulti:
    """reset(seed) gives every env its stream; the crowded state replaces the board."""
    o = OracleMulti(shape.oracle_params(), E)
    o.reset(seed + np.arange(E))
    o.set_state(*(init[k] for k in ("ground", "order", "y", "x", "charge", "packet")))
    return o


@functools.lru_cache(maxsize=None)
def trajectory(shape_id: str, seed: int) -> Trajectory:
    """The oracle's run over a shape's crowded states; computed once per
    process, shared by every test and never modified."""
    shape = BY_ID[shape_id]
    init = generate(shape, seed)
    o = seeded_oracle(shape, seed, init)
    N = shape.n
    states = [o.state()]
    rewards = np.zeros((STEPS, E, N), np.float64)
    dones = np.zeros((STEPS, E, N), bool)
    used = np.zeros((STEPS, E), np.int64)
    error = None
    for t in range(STEPS):
        try:
            rewards[t], dones[t] = o.step(init["actions"][t])
        except oracle.NoFreeCell as ex:
            error = f"step {t}: {ex}"
            break
        states.append(o.state())
        for e in range(E):
            used[t, e] = entries_used(shape.side, states[t]["mt"][e], states[t + 1]["mt"][e])
    for a in (rewards, dones, used):
        a.setflags(write=False)
    return Trajectory(shape, seed, init, init["actions"], states, rewards, dones, used, error)
