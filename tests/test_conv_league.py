"""A league of conv learners: K conv DQN learners trained against each other
in shared envs, learner k on drone index k -- drl_convleague_*
(dronerl_amd/csrc/convleague/), dronerl_amd.league.ConvLeagueDQN,
train_league(network_type="conv") and `python -m dronerl_amd.conv_league`.

Reference: torch_impl/helpers/rl_helpers.py:21-65 (MultiAgentTrainer.train);
each learner is train_jax.py:38-115's learner block with network_type 'conv'
on its own drone.

The yardsticks are code that exists without the conv league:
tests/_conv_pop_ref.py (a numpy restatement of cl_forward's summation order),
drl_convpop_act (unchanged), the two action hashes and
train_population(network_type="conv").  Every GPU comparison is BIT FOR BIT:
no tolerance anywhere; the learning test asserts an ordering only."""
import ctypes
import glob
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import dqn_learner as O
from test_conv_population import SHAPES as POP_SHAPES
from test_conv_population import _bits, _desc, _host
from test_dqn import _hash_explore
from tests import _conv_learner_ref as R
from tests import _conv_pop_ref as F32

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
MODELS = os.path.join(HERE, "golden", "sample_models")
vp = ctypes.c_void_p
# the envs of test_conv_population.SHAPES; h (W 9) runs in c's
SHAPES = dict(POP_SHAPES, h=POP_SHAPES["c"])
PLAN_NETS = ("a", "b", "c", "g", "h", "i")
ENV_TILES = (16, 8, 4, 2)


def _lib():
    from dronerl_amd._native import lib
    from dronerl_amd.dqn import _bind, _bind_convnet
    from dronerl_amd.league import _bind_convleague
    from dronerl_amd.population import _bind_convpop, _bind_pop
    return _bind_convleague(_bind_convpop(_bind_pop(_bind(_bind_convnet(lib())))))


# ------------------------------------------------------------------- CPU ---
def test_convleague_calls_validate_before_device_work():
    """drl_convleague_act and the plan query are refused before any device
    work (no GPU), with the reason in drl_last_error: NULL descriptor, plan,
    block, codes or actions; a misaligned block or codes; members 0 and
    members > n_drones; n_drones 0 and 65; num_envs 0; an f32-input
    descriptor; window 3."""
    from dronerl_amd.dqn import convnet_desc
    from dronerl_amd.league import DrlConvLeagueActPlan
    L = _lib()
    E = L.drl_last_error
    good = _desc("b")
    blk, ptr = vp(1 << 20), vp(1 << 21)
    odd = vp((1 << 21) + 8)
    w3 = convnet_desc((3, 3, 6), (R._c(8, 1, 1, 0),), (8,), 5, "code")

    def act(d=good, K=3, B=8, pop=blk, codes=ptr, E_=4, acts=ptr, N=4, q=None):
        return L.drl_convleague_act(None if d is None else ctypes.byref(d), K, B, pop, codes, E_, 0, 0, 0, 0, acts, N,
                                    q, None)

    assert act(d=None) != 0 and b"NULL" in E()
    for K, N in ((0, 4), (-1, 4), (5, 4), (65, 64), (2, 1)):
        assert act(K=K, N=N) != 0 and b"members" in E(), (K, N, E())
    assert act(N=0) != 0 and b"n_drones" in E()
    assert act(N=65) != 0 and b"n_drones" in E()
    assert act(E_=0) != 0 and b"num_envs" in E()
    assert act(E_=-3) != 0 and b"num_envs" in E()
    assert act(K=4, N=4, E_=1 << 29) != 0 and b"num_envs" in E()
    assert act(d=_desc("b", "obs")) != 0 and b"policy code" in E()
    assert act(d=w3) != 0 and b"window" in E()
    assert act(d=_desc("b", n_actions=9)) != 0 and b"n_actions" in E()
    assert act(B=0) != 0 and b"max_batch" in E()
    assert act(pop=None) != 0 and b"population block" in E()
    assert act(pop=vp((1 << 20) + 8)) != 0 and b"16-byte" in E()
    assert act(codes=None) != 0 and b"policy codes" in E()
    assert act(codes=odd) != 0 and b"16-byte" in E()
    assert act(acts=None) != 0 and b"actions" in E()
    assert act(q=vp((1 << 21) + 2)) != 0 and b"4-byte" in E()
    # the plan query
    plan = DrlConvLeagueActPlan()
    assert L.drl_convleague_act_plan_query(None, ctypes.byref(plan)) != 0 and b"NULL" in E()
    assert L.drl_convleague_act_plan_query(ctypes.byref(good), None) != 0 and b"plan is NULL" in E()
    assert L.drl_convleague_act_plan_query(ctypes.byref(_desc("b", "obs")), ctypes.byref(plan)) != 0 and b"policy code" in E()
    assert L.drl_convleague_act_plan_query(ctypes.byref(w3), ctypes.byref(plan)) != 0 and b"window" in E()
    assert L.drl_convleague_act_plan_query(ctypes.byref(good), ctypes.byref(plan)) == 0 and plan.env_tile in ENV_TILES


def test_convleague_act_plan_fits_and_places_every_word_once(tmp_path):
    """tests/native/convleague_layout_check.cpp, a stand-alone program under
    the address and undefined-behaviour sanitizers (nothing is loaded into
    Python), sweeps the descriptors cg::plan accepts (the file states the
    grid): the plan's LDS stays within 160 KiB, the env tile is the largest
    of 16, 8, 4, 2 that fits and 2 is never refused, the forward-only rows
    place every input, activation and head word once.  The numbers the Python
    layer reads (drl_convleague_act_plan_query) equal the ones the header
    gives the kernel."""
    from dronerl_amd.league import conv_act_plan
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "convleague_layout_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(HERE, "native", "convleague_layout_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    # 3 windows x (81 + 81^2) conv choices x 4 dense tails; cg::plan refuses 8,438 of them
    assert "grid 79704, accepted 71266," in r.stdout
    seen = {}
    for line in r.stdout.splitlines():
        if line.startswith("PLAN"):
            key, val = line[5:].split(" : ")
            seen[key] = tuple(int(v) for v in val.split())
    assert set(PLAN_NETS) <= set(seen)
    for name in PLAN_NETS:
        p = conv_act_plan(_desc(name))
        assert seen[name] == (p["env_tile"], p["threads"], p["row_words"], p["lds_bytes"]), (name, p)
        assert p["lds_bytes"] == p["env_tile"] * p["row_words"] * 4 <= p["lds_limit"] == 160 * 1024
        assert p["env_tile"] in ENV_TILES and p["threads"] % 256 == 0 and 256 <= p["threads"] <= 1024


def test_conv_league_cli_refusals_grid_and_opponents():
    """conv_league.parse_args: the grid maps to learners (K points or one
    shared), --opponents' words map to drone indices, the conv options
    arrive, and the refusals are raised; train_league refuses an unknown
    network_type; dronerl_amd.league keeps refusing conv and names this
    command."""
    from dronerl_amd import EnvParams, conv_league, league
    with pytest.raises(ValueError, match="dronerl_amd.league"):
        conv_league.parse_args(["--network_type", "dense"])
    with pytest.raises(ValueError, match="one GPU.*use_sharding"):
        conv_league.parse_args(["--use_sharding", "--num_envs", "8"])
    with pytest.raises(ValueError, match="more learners than drones"):
        conv_league.parse_args(["--learners", "5", "--n_drones", "4"])
    with pytest.raises(ValueError, match="learners must be >= 1"):
        conv_league.parse_args(["--learners", "0"])
    with pytest.raises(ValueError, match="opponent index 1 is below the number of learners"):
        conv_league.parse_args(["--learners", "2", "--opponents", "1=a.safetensors"])
    with pytest.raises(ValueError, match="not valid JSON"):
        conv_league.parse_args(["--grid", "{gamma: 1}"])
    with pytest.raises(ValueError, match="3 points: one per learner .2. or one shared"):
        conv_league.parse_args(["--grid", '{"gamma": [0.9, 0.8, 0.7]}'])
    with pytest.raises(ValueError, match="learners are dense nets.*dronerl_amd.conv_league.*conv checkpoints work"):
        league.parse_args(["--network_type", "conv"])
    with pytest.raises(ValueError, match="network_type"):
        league.train_league(EnvParams(), [], 1, 1, network_type="nope")
    args, points = conv_league.parse_args([
        "--learners", "2", "--grid", '{"learning_rate": [1e-4, 5e-4]}', "--n_drones", "6", "--grid_size", "11",
        "--num_envs", "64", "--num_steps", "40", "--seed", "5", "--gamma", "0.8", "--opponents", "a.st", "b.st",
        "5=c.st", "--conv_layers",
        '[{"out_channels": 16, "kernel_size": 3, "padding": 1}, {"out_channels": 32, "kernel_size": 3, "padding": 1}]',
        "--conv_dense_layers", "128", "64"])
    hps = league.learners_of(args, points)
    assert [hp.learning_rate for hp in hps] == [1e-4, 5e-4] and all(hp.gamma == 0.8 and hp.num_steps == 40 for hp in hps)
    assert [hp.sample_seed for hp in hps] == [5, 6]
    assert (args.network_type, args.learners, args.num_envs) == ("conv", 2, 64)
    assert [c["out_channels"] for c in args.conv_layers] == [16, 32] and tuple(args.conv_dense_layers) == (128, 64)
    assert args.opponents == {2: "a.st", 3: "b.st", 5: "c.st"}  # (drone 4 is random)
    a2, p2 = conv_league.parse_args(["--learners", "3", "--grid", '{"batch_size": [16]}'])
    assert [hp.batch for hp in league.learners_of(a2, p2)] == [16, 16, 16] and a2.opponents == {}
    assert len(a2.conv_layers) == 1 and a2.conv_layers[0]["out_channels"] == 8  # train_jax's default conv net
    a3, p3 = conv_league.parse_args(["--learners", "4", "--grid", '{"batch_size": [8, 16], "tau": [1.0, 0.5]}',
                                     "--network_type", "conv"])
    assert [(hp.batch, hp.tau) for hp in league.learners_of(a3, p3)] == [(8, 1.0), (8, 0.5), (16, 1.0), (16, 0.5)]


# Every __global__ kernel under csrc/convleague/ and the -m gpu test that launches it.
KERNEL_TESTS = {
    "drl_convleague_act_kernel": "test_conv_league.py::test_convleague_act_is_the_learners_forward_bit_exact",
}


def test_every_convleague_kernel_has_a_gpu_test():
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "convleague", "*.hip")):
        src = open(f).read()
        for m in re.finditer(r"__global__", src):
            k = re.search(r"\b(drl_[a-z0-9_]+_kernel)\s*\(", src[m.end():m.end() + 300])
            if k:
                found.add(k.group(1))
    assert found == set(KERNEL_TESTS), (sorted(found - set(KERNEL_TESTS)), sorted(set(KERNEL_TESTS) - found))
    text = open(__file__).read()
    for kern, ref in KERNEL_TESTS.items():
        fname, test = ref.split("::")
        assert fname == os.path.basename(__file__)
        assert re.search(rf"^@gpu\n(?:@pytest[^\n]*\n(?:[ \t]+[^\n]*\n)*)*def {test}\(", text, re.M), (kern, ref)


# ------------------------------------------------------------------- GPU ---
def _rand_sets(name, K, seed):
    """Per learner ([W], [b]) with random weights AND biases, online and target (tests/_conv_learner_ref.py)."""
    W, conv, dense = R.NETS[name]

    def one(s):
        ws, bs = zip(*R.random_params(W, conv, dense, s))
        return [torch.tensor(w) for w in ws], [torch.tensor(b) for b in bs]
    return [one(seed + 2 * k) for k in range(K)], [one(seed + 2 * k + 1) for k in range(K)]


def _np_online(lg, k):
    return [(_host(w), _host(b)) for w, b in lg.params("online", k)]


@gpu
@pytest.mark.parametrize("K", [1, 3, "N"])
@pytest.mark.parametrize("name", ["b", "c", "g", "i", "h"])
def test_convleague_act_is_the_learners_forward_bit_exact(name, K):
    """K learners with different random weights and biases and epsilons 0, 1,
    0.3, 0.7, ..., at E = 1, T - 1, T, T + 1 and 3 T + 5 envs (T: the kernel's
    env tile, from the plan query), three random env steps in: learner k's Q
    of env i equals tests/_conv_pop_ref.forward on the decoded row
    codes[k, i] bit for bit, laid out [K][E][A], and equals drl_convpop_act's
    q_out on the same K * E rows bit for bit; its action is the explore draw
    of the stream seed + k at (step, env_offset + i) or the first argmax of
    that Q; the action matrix was filled with a sentinel and Q with NaN:
    columns >= K keep it, as do the 64 words behind both buffers; the greedy
    flag ignores epsilon."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.evaluator import obs_code_all
    from dronerl_amd.league import ConvLeagueDQN, conv_act_plan
    from dronerl_amd.population import ConvPopulationDQN
    W, conv, dense = R.NETS[name]
    ep = EnvParams(**SHAPES[name])
    N, A = ep.n_drones, 5
    K = N if K == "N" else K
    T = conv_act_plan(_desc(name))["env_tile"]
    assert T in ENV_TILES
    eps = ([0.0, 1.0, 0.3, 0.7] * 2)[:K]
    hps = [DQNHParams(batch=8, epsilon_start=e, epsilon_decay=1.0, epsilon_end=0.0) for e in eps]
    online, target = _rand_sets(name, K, 13)
    SENT = 0x5A5A5A5A
    for E in (1, T - 1, T, T + 1, 3 * T + 5):
        env = BatchedDeliveryDrones(ep, E, env_offset=1000)
        env.reset(seed=2)
        for t in range(3):  # (a few random steps: drones in the windows, charges below 100)
            env.step(env.synth_actions(9, t))
        codes = obs_code_all(env)
        lg = ConvLeagueDQN((W, W, 6), conv, dense, hps, E, online=online, target=target)
        assert lg.act_plan["env_tile"] == T
        abuf = torch.full((E * N + 64,), SENT, dtype=torch.int32, device="cuda")
        qbuf = torch.full((K * E * A + 64,), float("nan"), dtype=torch.float32, device="cuda")
        acts, q = abuf[:E * N].view(E, N), qbuf[:K * E * A].view(K, E, A)
        lg.act(codes, 6, seed=3, env_offset=env.env_offset, actions=acts, q=q)
        a_h, q_h, c_h = _host(acts), _host(q), _host(codes)
        # drl_convpop_act (unchanged) on the same K * E rows: a population of K members with E envs each
        qpop = torch.full((K * E, A), float("nan"), dtype=torch.float32, device="cuda")
        ConvPopulationDQN.act(lg, codes[:K].reshape(K * E, -1).contiguous(), 6, seed=3, q_out=qpop)
        assert np.array_equal(_bits(_host(qpop)).reshape(K, E, A), _bits(q_h)), ("convpop Q", E)
        want = []
        for k in range(K):
            qk = F32.forward(_np_online(lg, k), conv, O.decode_code_rows(c_h[k], W), W)
            want.append(qk)
            assert np.array_equal(_bits(q_h[k]), _bits(qk)), ("Q", E, k, np.abs(q_h[k] - qk).max())
            for i in range(E):
                explore, rnd = _hash_explore(3 + k, 6, 1000 + i, A, eps[k])
                assert a_h[i, k] == (rnd if explore else int(np.argmax(qk[i]))), (E, k, i)
        assert (a_h[:, K:] == SENT).all(), E
        assert bool((abuf[E * N:] == SENT).all()) and bool(torch.isnan(qbuf[K * E * A:]).all()), E
        # greedy: the argmax everywhere, whatever epsilon holds; no Q buffer
        abuf.fill_(SENT)
        lg.act(codes, 6, seed=3, env_offset=env.env_offset, actions=acts, greedy=True)
        g_h = _host(acts)
        for k in range(K):
            assert np.array_equal(g_h[:, k], np.argmax(want[k], axis=1).astype(np.int32)), ("greedy", E, k)
        assert (g_h[:, K:] == SENT).all() and bool((abuf[E * N:] == SENT).all()), E


@gpu
def test_conv_league_of_one_is_the_conv_population():
    """train_league(network_type="conv") with one learner and random others
    against train_population(network_type="conv") with P = 1 (same seeds, net
    b, N = 4, 9x9, E = 3, capacity 20, 15 steps, reset_env_every 6): every
    step's actions, rewards and dones, and at the end the block (parameters,
    Adam state, counters, scratch, records), the counters, the ring, the
    cursor and the size, are bit-identical."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.league import ConvLeagueDQN, train_league
    from dronerl_amd.population import train_population
    ep = EnvParams(n_drones=4, grid_size=9, window_radius=3)
    hp = DQNHParams(batch=4, num_steps=15, sample_seed=3, target_update_interval=2, epsilon_decay_every=1)
    kw = dict(reset_env_every=6, memory_size=20, seed=4, env_offset=40, action_seed=11, act_seed=5, seeds=[9],
              network_type="conv", conv_layers=R.NETS["b"][1], conv_dense_layers=())
    got, want = [], []
    a = train_league(ep, [hp], 3, 15, on_step=lambda t, p, rb, ac, rw, dn: got.append([_host(v) for v in (ac, rw, dn)]), **kw)
    b = train_population(ep, [hp], 3, 15, on_step=lambda t, p, rb, ac, rw, dn: want.append([_host(v) for v in (ac, rw, dn)]),
                         **kw)
    assert isinstance(a.league, ConvLeagueDQN)
    assert len(got) == len(want) == 15
    for t, (x, y) in enumerate(zip(got, want)):
        assert all(u.shape == v.shape and u.tobytes() == v.tobytes() for u, v in zip(x, y)), t
    assert torch.equal(a.league.block, b.pop.block)
    assert a.league.counters(0) == b.pop.counters(0) and a.league.counters(0)["count"] > 0
    for key, v in a.replay.ring(0).items():
        assert torch.equal(v, b.replay.ring(0)[key]), key
    assert (a.replay.cursor, a.replay.size) == (b.replay.cursor, b.replay.size)


@gpu
def test_conv_league_loop_matches_a_host_loop():
    """K = 3 conv learners (net i) with different hyperparameters (batches 4,
    6, 9; different lr, tau, gamma, epsilon schedules), one random drone,
    N = 4, E = 2, 30 steps, reset_env_every 10, capacity 24, stepped as
    train_league steps them.  Through on_step (between step t's add and its
    train): learner k's actions equal tests/_conv_pop_ref.forward on that
    step's parameter snapshot and the codes the act read, plus the explore
    hash at the snapshot's epsilon; the random drone's column is the
    synthetic stream.  At the end each ring equals a numpy ring built from
    the recorded codes, actions, rewards and dones, and the train counts are
    [29, 28, 26] (size >= batch)."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.league import ConvLeagueDQN, LeagueLoop, LeagueReplay
    from oracle.oracle import synth_actions
    K, E, steps, cap, seed, aseed, sseed, A, N = 3, 2, 30, 24, 3, 7, 2024, 5, 4
    W, conv, dense = R.NETS["i"]
    ep = EnvParams(n_drones=N, grid_size=9, window_radius=3)
    hps = [DQNHParams(batch=4, num_steps=steps, sample_seed=1, target_update_interval=2),
           DQNHParams(batch=6, num_steps=steps, sample_seed=2, learning_rate=3e-3, tau=0.5, epsilon_decay_every=2),
           DQNHParams(batch=9, num_steps=steps, sample_seed=3, gamma=0.8, epsilon_end=0.2, epsilon_decay_every=1)]
    env = BatchedDeliveryDrones(ep, E)
    env.reset(seed=seed)
    lg = ConvLeagueDQN((W, W, 6), conv, dense, hps, E, seeds=[5, 9, 13])
    rb = LeagueReplay(K, cap, ep.window_radius)
    loop = LeagueLoop(env, lg, rb, {}, action_seed=sseed, act_seed=aseed)
    seen = []

    def on_step(t, league, replay, acts, rew, don):
        seen.append(dict(prev=_host(loop.codes[loop.cur]), nxt=_host(loop.codes[1 - loop.cur]), acts=_host(acts),
                         rew=_host(rew), don=_host(don), params=[_np_online(league, k) for k in range(K)],
                         eps=[league.counters(k)["epsilon"] for k in range(K)]))

    for t in range(steps):
        loop.step(t, on_step=on_step, reset=t % 10 == 0)
    torch.cuda.synchronize()
    env.check_errors()
    CB = env.policy_code_bytes
    rings = [dict(obs=np.zeros((cap, CB), np.uint8), next_obs=np.zeros((cap, CB), np.uint8),
                  actions=np.zeros(cap, np.int32), rewards=np.zeros(cap, np.float32), dones=np.zeros(cap, np.uint8))
             for _ in range(K)]
    cursor = size = 0
    explored = 0
    for t, s in enumerate(seen):
        want = synth_actions(sseed, t, np.arange(E), N)
        for k in range(K):
            q = F32.forward(s["params"][k], conv, O.decode_code_rows(s["prev"][k], W), W)
            for i in range(E):
                explore, rnd = _hash_explore(aseed + k, t, i, A, s["eps"][k])
                explored += int(explore)
                want[i, k] = rnd if explore else int(np.argmax(q[i]))
        assert np.array_equal(s["acts"], want), ("actions", t)
        for k in range(K):
            for i in range(E):
                at = (cursor + i) % cap
                rings[k]["obs"][at], rings[k]["next_obs"][at] = s["prev"][k, i], s["nxt"][k, i]
                rings[k]["actions"][at], rings[k]["rewards"][at] = s["acts"][i, k], s["rew"][i, k]
                rings[k]["dones"][at] = s["don"][i, k]
        cursor, size = (cursor + E) % cap, min(size + E, cap)
    assert 0 < explored < K * E * steps  # (both branches of the action rule were taken)
    for k in range(K):
        got = {key: _host(v) for key, v in rb.ring(k).items()}
        for key in ("obs", "next_obs", "actions", "dones"):
            assert np.array_equal(got[key], rings[k][key]), (k, key)
        assert np.array_equal(_bits(got["rewards"]), _bits(rings[k]["rewards"])), k
    assert (rb.cursor, rb.size) == (cursor, size)
    assert [lg.counters(k)["count"] for k in range(K)] == [29, 28, 26]


@gpu
def test_conv_league_step_replays_from_a_captured_graph():
    """One captured league step -- synthetic columns, the conv league act, a
    fixed dense opponent's act, the env step, every drone's code, the add,
    train -- replayed 4 times equals 4 eager steps (K = 2, N = 4, net b,
    E = 5): block, rings and actions bit-identical.  The host's part of a
    step is frozen by a capture, so both runs keep it fixed: the act's step
    argument, the ring's cursor, no refill."""
    from dronerl_amd import BatchedDeliveryDrones, EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.evaluator import obs_code_all
    from dronerl_amd.league import ConvLeagueDQN, LeagueLoop, LeagueReplay, resolve_opponents
    E, cap, k, K = 5, 64, 4, 2
    W, conv, dense = R.NETS["b"]
    hps = [DQNHParams(batch=3, sample_seed=1, epsilon_decay=0.9, epsilon_decay_every=1),
           DQNHParams(batch=8, sample_seed=2, tau=0.5, target_update_interval=2, learning_rate=3e-3)]
    online, target = _rand_sets("b", K, 31)
    ep = EnvParams(**SHAPES["b"])
    path = {2: os.path.join(MODELS, "dqn-agent-2.safetensors")}

    def fresh():
        env = BatchedDeliveryDrones(ep, E)
        env.reset(seed=6)
        lg = ConvLeagueDQN((W, W, 6), conv, dense, hps, E, online=online, target=target)
        rb = LeagueReplay(K, cap, ep.window_radius)
        env.refill_every = 0  # (where the respawn draws happen, never what they are)
        loop = LeagueLoop(env, lg, rb, resolve_opponents(path, K, ep, env.device), action_seed=5, act_seed=3)
        assert loop.any_random
        loop.step(0)
        loop.step(1)  # (back on code buffer 0; ten rows: both learners train; the fixed net's act has run once)
        c0, s0 = rb.cursor, rb.size
        cur, nxt = loop.codes[0], loop.codes[1]

        def step():
            loop.cur = 0
            loop.act(9)
            env.step(loop.actions, rewards=loop.rewards, dones=loop.dones)
            obs_code_all(env, nxt)
            rb.cursor, rb.size = c0, s0
            rb.add(cur, loop.actions, loop.rewards, nxt, loop.dones)
            lg.train(rb)
            cur.copy_(nxt)
        return env, lg, rb, loop, step

    env, lg, rb, loop, step = fresh()
    for _ in range(k):
        step()
    torch.cuda.synchronize()
    env2, lg2, rb2, loop2, step2 = fresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            step2()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(k):
        g.replay()
    torch.cuda.synchronize()
    env2.check_errors()
    assert torch.equal(lg.block, lg2.block)  # (parameters, counters, scratch and records alike)
    assert torch.equal(loop.actions, loop2.actions) and torch.equal(loop.codes[0], loop2.codes[0])
    assert torch.equal(loop.rewards, loop2.rewards) and torch.equal(loop.dones, loop2.dones)
    for key in ("obs", "next_obs", "actions", "rewards", "dones"):
        assert torch.equal(getattr(rb, key), getattr(rb2, key)), key
    d1, d2 = env.decode(), env2.decode()
    assert all(torch.equal(d1[key], d2[key]) for key in d1)
    assert [lg2.counters(m)["count"] for m in range(K)] == [k + 2, k + 1]  # (step 0 held five rows: only batch 3 trained)
    assert lg2.counters(0)["epsilon"] < 0.9 ** k  # (every replay decayed the device epsilon the next one read)


@gpu
def test_conv_league_learners_beat_the_random_drones():
    """Two conv learners (train_jax's default conv net) and two random
    drones, 9x9, 4,096 envs, 300 steps at batch 256; in evaluate_league's
    greedy table (5 episodes of 1,000 steps) each learner's mean episode
    reward is above the random drones' mean.  The condition is the ordering
    only.  Measured on an MI355X (the run is deterministic): learners -65.4
    and -62.5, random drones -178.4 and -180.6 per 1,000-step episode."""
    from dronerl_amd import EnvParams
    from dronerl_amd.dqn import DQNHParams
    from dronerl_amd.league import evaluate_league, train_league
    ep = EnvParams(n_drones=4, grid_size=9, window_radius=3)
    hps = [DQNHParams(batch=256, num_steps=300, sample_seed=s) for s in (0, 1)]
    res = train_league(ep, hps, 4096, 300, seeds=[0, 1], network_type="conv")
    assert [res.league.counters(k)["count"] for k in range(2)] == [300, 300]
    ev = evaluate_league(res, num_steps=1000)
    print("conv league eval, mean episode reward per drone:", [round(float(v), 2) for v in ev["mean"]], ev["roles"])
    assert ev["scores"].shape == (5, 4) and ev["roles"] == ["learner 0", "learner 1", "random", "random"]
    rnd = float(ev["mean"][2:].mean())
    assert float(ev["mean"][0]) > rnd and float(ev["mean"][1]) > rnd, ev["mean"]


@gpu
def test_conv_league_cli_end_to_end(tmp_path, capsys):
    """Two conv learners (4 x 3 x 3 + dense 8) against a dense and the conv
    sample baseline on a tiny run: the JSON line parses, roles and train
    counts are right, K x 2 checkpoints are written and reload through
    checkpoint.to_qnet as conv nets of that shape."""
    from dronerl_amd import conv_league
    from dronerl_amd.checkpoint import read_checkpoint, to_qnet
    from dronerl_amd.dqn import ConvQNetwork
    out = conv_league.main(["--learners", "2", "--opponents", os.path.join(MODELS, "dqn-agent-1.safetensors"),
                            os.path.join(MODELS, "dqn-agent-5.safetensors"), "--n_drones", "4", "--grid_size", "9",
                            "--num_envs", "8", "--num_steps", "30", "--conv_layers",
                            '[{"out_channels": 4, "kernel_size": 3, "padding": 1}]', "--conv_dense_layers", "8",
                            "--grid", '{"learning_rate": [1e-3, 3e-3]}', "--num_evals", "2", "--num_eval_steps", "50",
                            "--save_final_checkpoint", "--output_dir", str(tmp_path)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["learners"] == 2 and line["steps_per_sec"] > 0 and len(line["eval"]) == 4
    assert line["network_type"] == "conv" and line["conv_dense_layers"] == [8]
    assert [r["role"] for r in line["eval"]] == ["learner 0", "learner 1", "opponent", "opponent"]
    assert all(np.isfinite([r["reward_mean"], r["reward_std"]]).all() for r in line["eval"])
    assert [r["train_steps"] for r in line["eval"][:2]] == [30, 30]
    assert len(out["checkpoints"]) == 2
    for k, paths in enumerate(out["checkpoints"]):
        for fmt in ("jax", "torch"):
            net = to_qnet(read_checkpoint(paths[fmt]))
            assert isinstance(net, ConvQNetwork), (k, fmt)
            assert [tuple(w.shape) for w in net.conv_weights] == [(4, 6, 3, 3)], (k, fmt)
            assert [tuple(w.shape) for w in net.weights] == [(8, 196), (5, 8)], (k, fmt)
            assert all(bool(torch.isfinite(w).all()) for w in (*net.conv_weights, *net.weights))
