"""Multi-agent line-up evaluation: drl_obs_code_all, drl_score_add and dronerl_amd.evaluator.

CPU: argument refusals before any device work, the env-index / act-range plan, CPython's seed words, the reward ->
double map against compat._py_reward, the refusal of ambiguous rewards, the score recurrence in numpy, and the
kernel -> GPU-test manifest of csrc/evalcode/.

GPU: (1) code rows on crowded boards against get_code / get_obs / an env with two drone indices swapped, (2) the
score kernel against numpy's float64 recurrence, (3) the reference evaluator's table reproduced exactly with the
torch-CPU nets as host callables, (4) device nets checked against torch's argmax wherever its top-2 gap is clear,
(5) batching, (6) two gloo ranks == one process, (7) the command line.
"""
import ctypes
import json
import os
import random
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from dronerl_amd import EnvParams
from dronerl_amd import evaluator as ev
from dronerl_amd._native import DrlState, lib
from dronerl_amd.compat import _py_reward

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
MODELS = os.path.join(GOLD, "sample_models")
SEEDS = list(ev.EPISODE_SEEDS)
PUBLISHED_1 = (-64.98, 6.109)  # test_drone_evaluator.py:5-11, submission 1


def model(i):
    return os.path.join(MODELS, f"dqn-agent-{i}.safetensors")


# ------------------------------------------------------------------- CPU ---
def test_calls_refuse_bad_arguments_before_device_work():
    L, vp = lib(), ctypes.c_void_p
    good = EnvParams(n_drones=6, grid_size=11, window_radius=3).to_c()

    def code_all(p=good, s=DrlState(1024, 1024, 1024, 1024, 4), codes=vp(4096)):
        return L.drl_obs_code_all(None if p is None else ctypes.byref(p), None if s is None else ctypes.byref(s),
                                  codes, None)
    assert code_all(codes=None) != 0 and b"codes is NULL" in L.drl_last_error()
    assert code_all(codes=vp(4104)) != 0 and b"16-byte" in L.drl_last_error()
    assert code_all(s=None) != 0 and b"state is NULL" in L.drl_last_error()
    assert code_all(s=DrlState(1024, 1024, 1024, 1024, 0)) != 0 and b"num_envs" in L.drl_last_error()
    assert code_all(s=DrlState(1024, 1024, 1024, 1024, -3)) != 0 and b"num_envs" in L.drl_last_error()
    assert code_all(s=DrlState(None, 1024, 1024, 1024, 4)) != 0 and b"NULL" in L.drl_last_error()
    assert code_all(s=DrlState(1024, None, 1024, 1024, 4)) != 0 and b"NULL" in L.drl_last_error()
    assert code_all(s=DrlState(1032, 1024, 1024, 1024, 4)) != 0 and b"aligned" in L.drl_last_error()
    assert code_all(p=None) != 0 and b"NULL" in L.drl_last_error()
    for radius in (0, 9, -1):
        bad = EnvParams(n_drones=6, grid_size=11).to_c()
        bad.window_radius = radius
        assert code_all(p=bad) != 0 and b"window_radius" in L.drl_last_error()
    bad = EnvParams(n_drones=6, grid_size=11).to_c()
    bad.n_drones = 65
    assert code_all(p=bad) != 0 and b"n_drones" in L.drl_last_error()

    def score(rew=vp(1024), E=4, N=6, out=vp(2048)):
        return L.drl_score_add(rew, E, N, -1.0, -0.1, 0.0, 1.0, out, None)
    assert score(rew=None) != 0 and b"NULL" in L.drl_last_error()
    assert score(out=None) != 0 and b"NULL" in L.drl_last_error()
    assert score(E=0) != 0 and b"num_envs" in L.drl_last_error()
    assert score(E=-1) != 0 and b"num_envs" in L.drl_last_error()
    assert score(N=0) != 0 and b"n_drones" in L.drl_last_error()
    assert score(out=vp(2052)) != 0 and b"aligned" in L.drl_last_error()
    assert score(rew=vp(1026)) != 0 and b"aligned" in L.drl_last_error()


def test_env_index_and_act_plan():
    S = 3
    assert [ev.env_index(l, s, S) for l in range(2) for s in range(S)] == list(range(6))
    f, g = (lambda w: 0), (lambda w: 1)
    a1, a1_again = model(1), os.path.join(MODELS, ".", "dqn-agent-1.safetensors")  # one file, two spellings
    lineups = [[a1, f, None], [a1_again, g, None], [model(2), g, f]]
    agents, acts, any_random = ev.plan_acts(lineups, S, 3)
    assert agents == [a1, model(2), f, g] and any_random
    # drone 0: the shared path over line-ups 0-1 in ONE launch, then model 2; drone 1: f, then g over 1-2
    assert acts == [(0, 0, 0, 6), (0, 1, 6, 9), (1, 2, 0, 3), (1, 3, 3, 9), (2, 2, 6, 9)]
    # a rank's shard: clipped to its envs, local indices
    agents2, acts2, rnd2 = ev.plan_acts(lineups, S, 3, range(4, 9))
    assert agents2 == agents and rnd2
    assert acts2 == [(0, 0, 0, 2), (0, 1, 2, 5), (1, 3, 0, 5), (2, 2, 2, 5)]
    assert ev.plan_acts(lineups, S, 3, range(6, 9))[2] is False  # line-up 2 has no random drone
    # every (env, drone) is covered exactly once by a launch or by the random stream
    cover = np.zeros((9, 3), int)
    for d, _, lo, hi in acts:
        cover[lo:hi, d] += 1
    for li, lu in enumerate(lineups):
        for d, a in enumerate(lu):
            cover[li * S:(li + 1) * S, d] += a is None
    assert (cover == 1).all()
    with pytest.raises(ValueError, match="one agent per drone"):
        ev.plan_acts([[f, g]], S, 3)


@pytest.mark.parametrize("seed", [845, 0, 35, -7, 2**64 + 5, 123456789012345678901234567890])
def test_seed_words_equal_cpython_getstate(seed):
    random.seed(seed)
    st = random.getstate()
    w = ev.seed_words(seed)
    assert len(w) == 625 and tuple(w) == st[1] and w[624] == 624


REWARD_SETS = [
    dict(ev.EVALUATOR_ENV_PARAMS),
    dict(crash_reward=-1, charge_reward=-0.25, pickup_reward=0.5, delivery_reward=1),
    dict(crash_reward=1e6, charge_reward=-0.1, pickup_reward=0.1, delivery_reward=-2.5),
    dict(crash_reward=-1.0, charge_reward=-1, pickup_reward=0, delivery_reward=0.0),  # equal doubles are fine
]


@pytest.mark.parametrize("cfg", REWARD_SETS)
def test_reward_to_double_matches_py_reward(cfg):
    doubles = ev.reward_doubles(cfg)
    for v in [cfg[k] for k in ("crash_reward", "charge_reward", "pickup_reward", "delivery_reward")] + [0, -0.0, 0.3]:
        r = np.float32(v)  # what drl_step writes
        want = _py_reward(float(r), cfg)
        got = ev.reward_to_double(r, doubles)
        assert isinstance(got, float) and got == float(want) and np.array(got).tobytes() == np.array(
            float(want) + 0.0).tobytes(), (v, got, want)


def test_ambiguous_rewards_are_refused():
    near = float(np.nextafter(np.float64(-0.1), 0))  # another double, the same f32
    assert np.float32(near) == np.float32(-0.1) and near != -0.1
    with pytest.raises(ValueError, match="same float32"):
        ev.reward_doubles(dict(crash_reward=-0.1, charge_reward=near, pickup_reward=0, delivery_reward=1))
    with pytest.raises(ValueError, match="same float32"):
        ev.reward_doubles(EnvParams(pickup_reward=1.0 + 2.0**-40, delivery_reward=1.0))
    ev.reward_doubles(EnvParams(pickup_reward=1.0, delivery_reward=1.0))


def _numpy_scores(rewards_f32, cfg):
    """The reference's accumulation (drone_evaluator.py:101,165-167) over f32 rewards [T, E, N]."""
    T, E, N = rewards_f32.shape
    scores = np.zeros((E, N))
    for t in range(T):
        for e in range(E):
            scores[e] += np.array([_py_reward(float(v), cfg) for v in rewards_f32[t, e]])
    return scores


def _reward_columns(cfg, T, E, N, seed):
    vals = np.array([np.float32(cfg[k]) for k in ("crash_reward", "charge_reward", "pickup_reward",
                                                   "delivery_reward")] + [np.float32(0)], np.float32)
    return vals[np.random.RandomState(seed).randint(0, len(vals), (T, E, N))]


def test_score_recurrence_in_numpy():
    cfg = REWARD_SETS[1]
    rew = _reward_columns(cfg, 50, 4, 3, 0)
    doubles = ev.reward_doubles(cfg)
    scores = np.zeros((4, 3))
    for t in range(50):  # drl_score_add: one f64 add per element per call
        scores += np.vectorize(lambda r: ev.reward_to_double(r, doubles))(rew[t])
    assert scores.tobytes() == _numpy_scores(rew, cfg).tobytes()
    # the evaluator's -0.1 is not f32(-0.1) widened: summing the kernel's f32 rewards would not do
    cfg0 = REWARD_SETS[0]
    rew0 = _reward_columns(cfg0, 50, 4, 3, 1)
    wide = np.zeros((4, 3))
    for t in range(50):
        wide += rew0[t].astype(np.float64)
    assert _numpy_scores(rew0, cfg0).tobytes() != wide.tobytes()


# Every __global__ kernel under csrc/evalcode/ and the -m gpu test that launches it.
KERNEL_TESTS = {
    "drl_obs_code_all_kernel": "test_lineup_eval.py::test_code_rows",
    "drl_score_add_kernel": "test_lineup_eval.py::test_score_add_equals_numpy_recurrence",
}


def test_every_evalcode_kernel_has_a_gpu_test():
    import glob
    found = set()
    for f in glob.glob(os.path.join(REPO, "dronerl_amd", "csrc", "evalcode", "*.hip")):
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
        assert re.search(rf"^@gpu\n(?:@pytest[^\n]*\n)*def {test}\(", text, re.M), (kern, ref)


# ------------------------------------------------------------------- GPU ---
SHAPES = [(5, 1, 1), (8, 4, 2), (11, 6, 3), (16, 8, 3), (13, 11, 4), (33, 20, 3), (26, 33, 8), (128, 4, 3),
          (36, 64, 3)]
ENVS = (1, 3, 17, 65)


def _crowded_state(side, N, E, seed):
    """Dense boards (70 % filled), the first drones in the corners and on the walls, a third of the batteries
    low, half the drones carrying (tests/_crowded.py's recipe; numpy only)."""
    rs = np.random.RandomState([side, N, E, seed])
    GG = side * side
    codes, share = np.array([2, 3, 4, 5], np.uint8), [0.25, 0.15, 0.30, 0.30]
    ground = np.zeros((E, GG), np.uint8)
    pos = np.zeros((E, N), np.int64)
    order = np.zeros((E, N), np.int32)
    G1 = side - 1
    special = [0, G1 * side + G1, G1, G1 * side, side // 2, G1 * side + side // 2, (side // 2) * side,
               (side // 2) * side + G1]  # 4 corners, 4 wall cells
    for e in range(E):
        nfill = int(0.7 * GG)
        ground[e, rs.permutation(GG)[:nfill]] = codes[rs.choice(4, size=nfill, p=share)]
        ground[e, special] = np.where(ground[e, special] == 2, 5, ground[e, special])  # no drone inside a tower
        free = np.setdiff1d(np.flatnonzero(ground[e] != 2), special)
        cells = special[:N] + list(free[rs.permutation(len(free))[:max(0, N - len(special))]])
        pos[e] = np.array(cells)[rs.permutation(N)]
        order[e] = rs.permutation(N)
    low = rs.random_sample((E, N)) < 0.3
    charge = np.where(low, rs.randint(1, 21, (E, N)), rs.randint(1, 101, (E, N))).astype(np.int32)
    carry = (rs.random_sample((E, N)) < 0.5).astype(np.uint8)
    return dict(ground=ground, order=order, y=(pos // side).astype(np.int32), x=(pos % side).astype(np.int32),
                charge=charge, carrying=carry)


def _swapped(st, d):
    """The same board with drone indices d and 0 swapped (who stands where, and the dict order's labels)."""
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    for k in ("y", "x", "charge", "carrying"):
        out[k][:, [0, d]] = st[k][:, [d, 0]]
    o = np.array(st["order"], copy=True)
    out["order"] = np.where(o == 0, d, np.where(o == d, 0, o)).astype(np.int32)
    return out


def _host_state(env):
    dec = env.decode()
    E = env.num_envs
    return dict(ground=dec["ground"].cpu().numpy().reshape(E, -1), order=dec["order"].cpu().numpy(),
                y=dec["y"].cpu().numpy(), x=dec["x"].cpu().numpy(), charge=dec["charge"].cpu().numpy(),
                carrying=dec["carrying"].cpu().numpy())


def _set(env, st):
    env.set_state(st["ground"], st["order"], st["y"], st["x"], st["charge"], st["carrying"])


def _check_code_rows(env, env2, tag):
    from dronerl_amd.dqn import decode_policy_code
    N, E, cb, R = env.n_drones, env.num_envs, env.policy_code_bytes, env.params.window_radius
    pad = 256
    buf = torch.full((N * E * cb + 2 * pad,), 0xA5, dtype=torch.uint8, device=env.device)
    codes = ev.obs_code_all(env, out=buf[pad:pad + N * E * cb].view(N, E, cb))
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + N * E * cb:] == 0xA5).all()), tag
    assert torch.equal(codes[0], env.get_code()), tag
    obs = env.get_obs(N).reshape(E, N, -1)
    for d in range(N):
        dec = decode_policy_code(codes[d].contiguous(), R)
        assert torch.equal(dec.view(torch.int32), obs[:, d].contiguous().view(torch.int32)), (tag, d)
    st = _host_state(env)
    for d in sorted({1, N // 2, N - 1} - {0}):
        if d >= N:
            continue
        _set(env2, _swapped(st, d))
        assert torch.equal(codes[d], env2.get_code()), (tag, "swap", d)


@gpu
@pytest.mark.parametrize("side,N,R", SHAPES, ids=[f"g{s}_n{n}_r{r}" for s, n, r in SHAPES])
def test_code_rows(side, N, R):
    from dronerl_amd import BatchedDeliveryDrones
    p = EnvParams(n_drones=N, grid_size=side, window_radius=R)
    for E in ENVS:
        env = BatchedDeliveryDrones(p, E, device="cuda:0")
        env2 = BatchedDeliveryDrones(p, E, device="cuda:0")
        env.reset(seed=3)  # (valid streams for the steps' respawns)
        _set(env, _crowded_state(side, N, E, 0))
        _check_code_rows(env, env2, (E, "generated"))
        for t in range(5):
            env.step(env.synth_actions(seed=9, step=t))
        _check_code_rows(env, env2, (E, "after 5 steps"))


@gpu
@pytest.mark.parametrize("E,N", [(1, 1), (10, 6), (4097, 3)])
@pytest.mark.parametrize("cfg", REWARD_SETS[:2], ids=["evaluator", "charge-0.25_pickup0.5"])
def test_score_add_equals_numpy_recurrence(cfg, E, N):
    doubles = ev.reward_doubles(cfg)
    rew = _reward_columns(cfg, 50, E, N, E)
    dev = torch.device("cuda", 0)
    scores = torch.zeros((E, N), dtype=torch.float64, device=dev)
    drew = torch.from_numpy(rew).to(dev)
    for t in range(50):
        ev.score_add(drew[t], scores, doubles)
    want = np.zeros((E, N))
    step = np.vectorize(lambda r: _py_reward(float(r), cfg), otypes=[np.float64])
    for t in range(50):
        want += step(rew[t])
    assert scores.cpu().numpy().tobytes() == want.tobytes()


def _torch_agents(sub):
    """The nets of tests/test_evaluator_parity.agents_for(sub): YOU, baseline-1..5."""
    from dronerl_amd.checkpoint import load_qnetwork
    return [load_qnetwork(model(i)) for i in (sub, 1, 2, 3, 4, 5)]


def _golden_scores():
    return np.load(os.path.join(GOLD, "evaluator_scores.npz"))["scores"]


@gpu
def test_reference_table_exact_with_host_callables():
    """The reference evaluator's table for submission 1, exactly: seeding, drl_obs_code_all (the windows the
    torch-CPU nets see), the loop and drl_score_add, independent of the device nets' numerics."""
    def greedy_one_by_one(net):  # the reference's call, a window at a time (drone_evaluator.py:157-158)
        def f(windows):
            with torch.no_grad():
                return [int(net([w])[0].argmax().item()) for w in windows]
        return f
    lineup = [greedy_one_by_one(n) for n in _torch_agents(1)]
    params = EnvParams.from_torch_config(ev.EVALUATOR_ENV_PARAMS, window_radius=3)
    assert (params.side, params.n_drones) == (11, 6)
    scores = ev.evaluate_lineups(params, [lineup], SEEDS, 1000, device="cuda:0")
    assert scores.shape == (1, 10, 6) and scores.dtype == np.float64
    np.testing.assert_array_equal(scores[0], _golden_scores()[0])
    mean, std = PUBLISHED_1
    assert np.isclose(scores[0][:, 0].mean(), mean, rtol=1e-2) and np.isclose(scores[0][:, 0].std(), std, rtol=1e-2)


TEACHER_GAP = 1e-4       # torch's top-2 gap / max|Q| from which a device action must be torch's argmax
TEACHER_MAX_SKIPPED = 0.003  # at most this share of a submission's decisions may lie below the gap


@gpu
def test_device_nets_follow_the_teacher():
    """evaluate_submissions (submissions 1: dense, 5: conv; device code-input nets) over 10 seeds x 300 steps
    with the actions recorded; a host replay steps a second env with them and reads get_obs(6), so the
    torch-CPU nets see the same windows at every step.  Wherever torch's top-2 gap / max|Q| >= 1e-4 the
    device action is torch's argmax; at most 0.3 % of the 18,000 decisions per submission may lie below.  The
    scores equal the float64 recurrence over the replay's rewards bit for bit.  Measured on an MI355X: 19
    (submission 1) and 18 (submission 5) of 18,000 decisions below the gap, none of the others differing."""
    from dronerl_amd import BatchedDeliveryDrones
    subs, T, S, N = (1, 5), 300, len(SEEDS), 6
    res = ev.evaluate_submissions([model(s) for s in subs], baselines=MODELS, num_steps=T, device="cuda:0",
                                  record_actions=True)
    params = EnvParams.from_torch_config(ev.EVALUATOR_ENV_PARAMS, window_radius=3)
    env = BatchedDeliveryDrones(params, len(subs) * S, device="cuda:0")
    env.set_mt_words(np.array([ev.seed_words(s) for _ in subs for s in SEEDS], dtype=np.int64))
    env.reset(seed=None)
    teachers = [_torch_agents(s) for s in subs]
    acts = np.concatenate([r["actions"] for r in res], axis=1)  # [T, 2 * S, N]
    assert acts.shape == (T, len(subs) * S, N) and acts.dtype == np.int32
    want = np.zeros((len(subs) * S, N))
    skipped, wrong = np.zeros(len(subs), int), []
    for t in range(T):
        obs = env.get_obs(N).cpu()
        for i in range(len(subs)):
            for d in range(N):
                with torch.no_grad():
                    q = teachers[i][d](obs[i * S:(i + 1) * S, d])
                top = q.topk(2, dim=1).values
                clear = ((top[:, 0] - top[:, 1]) / q.abs().max(dim=1).values >= TEACHER_GAP).numpy()
                skipped[i] += int((~clear).sum())
                a = acts[t, i * S:(i + 1) * S, d]
                bad = clear & (a != q.argmax(dim=1).numpy())
                wrong += [(subs[i], t, int(e), d) for e in np.flatnonzero(bad)]
        r, _ = env.step(torch.from_numpy(acts[t]).to(env.device))
        r = r.cpu().numpy()
        for e in range(r.shape[0]):
            want[e] += np.array([_py_reward(float(v), ev.EVALUATOR_ENV_PARAMS) for v in r[e]])
    env.check_errors()
    print("decisions below the teacher gap per submission:", dict(zip(subs, skipped.tolist())), "of", T * S * N)
    assert not wrong, wrong[:10]
    assert (skipped <= TEACHER_MAX_SKIPPED * T * S * N).all(), skipped
    got = np.concatenate([r["scores"] for r in res], axis=0)
    assert got.tobytes() == want.tobytes()
    for r in res:
        assert r["score"] == r["scores"].mean(axis=0)[0] and r["score_secondary"] == r["scores"].std(axis=0)[0]


def _small_params():
    return EnvParams(n_drones=4, grid_size=9, window_radius=3, charge_reward=-0.25, pickup_reward=0.5)


def _device_nets():
    from dronerl_amd.dqn import ConvQNetwork, QNetwork
    g = torch.Generator().manual_seed(11)
    code = QNetwork(294, (32, 16), device="cuda:0", generator=g, input="code")
    bf16 = QNetwork(294, (32, 32), device="cuda:0", generator=g, precision="bf16", input="obs")
    conv = ConvQNetwork((7, 7, 6), ({"out_channels": 4, "kernel_size": 3, "stride": 1, "padding": 1},), (8,),
                        device="cuda:0", generator=g, input="code")
    return code, bf16, conv


@gpu
def test_batched_equals_single_env_calls():
    p, T, seeds = _small_params(), 40, [5, 99, -3]
    code, bf16, conv = _device_nets()
    lineups = [[code, bf16, conv, model(1)], [bf16, code, conv, model(1)]]
    scores, acts = ev.evaluate_lineups(p, lineups, seeds, T, device="cuda:0", record_actions=True)
    assert scores.shape == (2, 3, 4) and acts.shape == (T, 6, 4)
    assert len(np.unique(acts)) > 1 and np.abs(scores).sum() > 0
    for l in range(2):
        for s in range(3):
            one, a1 = ev.evaluate_lineups(p, [lineups[l]], [seeds[s]], T, device="cuda:0", record_actions=True)
            assert one[0, 0].tobytes() == scores[l, s].tobytes(), (l, s)
            np.testing.assert_array_equal(a1[:, 0], acts[:, ev.env_index(l, s, 3)])


@gpu
def test_random_drones_take_the_synthetic_stream():
    from dronerl_amd import BatchedDeliveryDrones
    p, T, seeds = _small_params(), 25, [1, 2, 3]
    code, bf16, _ = _device_nets()
    _, acts = ev.evaluate_lineups(p, [[code, None, None, bf16], [None, code, bf16, None]], seeds, T,
                                  device="cuda:0", action_seed=7, record_actions=True)
    env = BatchedDeliveryDrones(p, 6, device="cuda:0")
    for t in range(T):
        syn = env.synth_actions(7, t).cpu().numpy()
        np.testing.assert_array_equal(acts[t, :3, 1:3], syn[:3, 1:3])
        np.testing.assert_array_equal(acts[t][3:][:, [0, 3]], syn[3:][:, [0, 3]])
    assert ((acts >= 0) & (acts < 5)).all()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


SHARD_STEPS, SHARD_SEEDS = 30, [845, 99, 65]


def _shard_lineups():
    return [[model(1), model(5), None, model(3)], [model(5), model(1), model(3), None]]


def _shard_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out[rank] = ev.evaluate_lineups(_small_params(), _shard_lineups(), SHARD_SEEDS, SHARD_STEPS, device="cuda:0",
                                        action_seed=2, record_actions=True, rank=rank, world=world)
    finally:
        dist.destroy_process_group()


@gpu
def test_two_ranks_equal_one_process():
    import torch.multiprocessing as mp
    ref_s, ref_a = ev.evaluate_lineups(_small_params(), _shard_lineups(), SHARD_SEEDS, SHARD_STEPS, device="cuda:0",
                                       action_seed=2, record_actions=True)
    ctx = mp.get_context("spawn")
    with ctx.Manager() as man:
        out = man.dict()
        port = _free_port()
        procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
            assert p.exitcode == 0, p.exitcode
        res = dict(out)
    for r in range(2):
        s, a = res[r]
        assert s.tobytes() == ref_s.tobytes()
        np.testing.assert_array_equal(a, ref_a)


@gpu
def test_command_line_prints_json():
    r = subprocess.run([sys.executable, "-m", "dronerl_amd.evaluate", model(2), "--baselines", MODELS,
                        "--episodes", "2", "--steps", "50"], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    tab = np.array(d["scores"])
    assert d["model"] == model(2) and tab.shape == (2, 6) and (d["episodes"], d["steps"]) == (2, 50)
    assert d["score"] == tab.mean(axis=0)[0] and d["score_secondary"] == tab.std(axis=0)[0]
